/*
 * wavefront.hip -- the wavefront engine of the render path.
 *
 * Same per-lane code as the megakernel (rt_path.h, rt_trace.h) and the same film (film.h), same
 * pcg32 streams, therefore the same radiance per camera sample; what changes is
 * how work is laid out for 64-wide waves.  In the megakernel a lane owns a
 * pixel and, when its path needs shading while its neighbours still traverse,
 * it waits.  Here paths live in HBM (sized for 288 GB: 216 B per path -- two state copies of 100 B, wf_records.h, and the
 * hit record --, up to 2^29 paths = 116 GB in flight) and every kernel runs with all lanes doing the SAME kind
 * of work:
 *
 *   loop until no path is alive (the first pass computes the camera sample of src/main.cpp:41-46
 *   in the kernels instead of reading path state):
 *     wf_extend  persistent waves pull paths from the dense state array; a lane traces
 *                the path's shadow ray, then its continuation ray, writes one hit
 *                record, and is refilled as soon as enough lanes of its wave are idle
 *                (__ballot + one atomic per chunk of paths)   -> Accel::rayIntersect
 *     wf_shade   one lane per path: consume the shadow result, shade the closest hit
 *                (Integrator::Li state machine), write the surviving path with its
 *                next rays COMPACTED into the second state copy (ping-pong), so
 *                every pass streams dense arrays however many paths have died
 *   wf_finish  once a batch has few live paths left a small persistent grid walks them to their ends (a lane pulls path after
 *              path); in a call of several batches it does so on its own CUs BESIDE the next batch (wavefront_render, "tail overlap")
 *   film_gather / film_resolve (film.hip)  the finished samples sit tile-major in the
 *                film's store; the reconstruction filter and the block merge
 *                (ImageBlock::put, src/block.cpp:62-102) run as gathers
 *
 * A path vertex costs ONE iteration: its shadow ray (slot B) and continuation
 * ray (slot A) are traced in the same wf_extend pass, and the next wf_shade
 * first adds the emitter sample if B was unoccluded, then shades A's hit --
 * the order in which the megakernel and the CPU oracle accumulate.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <mutex>
#include <vector>

#include "wf_device.h"

namespace nrt {
/* wavefront_env.hip: wf_shade / wf_finish of scenes with an environment map -- MATSET kAnyBsdf | kTextured | kEnvLit (rt_path.h), the
   full record, path_mats / path_ems / path_mis.  They are that unit's kernels, so this unit's set is the set it had.  wf_buf, batch:
   this unit's WfBuf and WfBatch (wf_device.h, which both units include; the types live in each unit's unnamed namespace). */
void wf_env_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s);
void wf_env_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid, hipStream_t s);
/* wavefront_medium.hip: the same for contexts with a medium -- MATSET kAnyBsdf | kTextured | kMedium */
void wf_medium_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s);
void wf_medium_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid, hipStream_t s);
/* wavefront_lights.hip: the same for contexts with delta lights -- MATSET kAnyBsdf | kTextured | kDeltaLit, and that with kEnvLit or kMedium */
void wf_lights_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s);
void wf_lights_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid, hipStream_t s);
/* wavefront_grid_medium.hip: the same for contexts with a grid medium -- MATSET kAnyBsdf | kTextured | kMedium | kGridMedium, and that with kDeltaLit */
void wf_grid_medium_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s);
void wf_grid_medium_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid, hipStream_t s);
}

namespace {

/* The BVH2 node loop of wf_extend, hand-written for gfx950, on the 32-B node records of rt_nodeq.h:
 *
 *     do { if (trav_at_inner(tv)) trav_inner_step_q(sc, stack, tv, tc, top); } while (lanes at inner nodes >= repeat);
 *
 * (rt_trace.h; BoundingBox::rayIntersect of include/nori/bbox.h:323-350 for both children).  With 64-B nodes wf_extend was bound by
 * the number of vector-memory instructions a CU issues -- each occupies its address path for ~16 cycles however few lanes take
 * part, while the arithmetic and scalar pipes were half idle.  Measured by adding instructions of each kind to the node step
 * (-DNORI_EXP_SENS=n, ms per frame): one more global_load_dwordx4 +6.3, a dwordx2 +5.2, a dword +2.8 -- the same with four lanes
 * active as with all of them --, sixteen v_mov +1.7, sixteen s_mov +0.4, the LDS reads over again +0.8.  So the loop reads a node
 * in TWO loads where the 64-B record takes four, and pays for it in arithmetic: per plane one v_cvt_f32_u32 (SDWA: a 16-bit half of
 * a dword) and one v_fma, per axis two v_bfi that pick the dword with the near planes by the sign of the ray's direction.  On this
 * loop the same experiment reads: one more dwordx4 +0.8, sixteen v_mov +1.8, 64 idle cycles +1.2 -- the kernel now sits against the
 * vector ALU (~80 % busy), which is where a ray tracer without ray-tracing hardware belongs.
 * Written as assembly because the child selection is two v_cndmask on a scalar-side mask and two exec-masked LDS operations (push
 * where both children are hit, pop where none is) where the compiler builds three nested regions with their save / restore /
 * skip-branch triples, because the loads must not be widened, merged or re-ordered, and because the loop's exit test can then look
 * ahead: it stays inside while the trip around the outer loop would run neither a triangle step nor a refill.
 * Same operations in the same order as trav_inner_step_q -- the CPU harness walks that one, against the linear scan.
 * gfx950 hazards honoured by hand: a VALU-written vcc is read by v_cndmask two instructions later at the earliest.
 * Records are addressed as base + (node << 5) in 32 bits: the caller takes this path for trees below 2^25 nodes only. */
#define NORI_SDWA(dst, src, half) "v_cvt_f32_u32_sdwa " dst ", " src " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_" half "\n\t"
/* CHECK_FULL (trees deeper than the LDS stack, LdsStackHybrid): before a step, lanes whose LDS stack is full (top >= stack_limit)
   end the loop -- returns true, and the caller does that step in C++. */
template <int STACK_STRIDE, bool CHECK_FULL>      /* STACK_STRIDE: bytes between a lane's stack slots */
__device__ __forceinline__ bool bvh2q_node_loop_asm(int &node_io, uint32_t &stack_top, float tmax, const NodeqRay &R, int mx, int my, int mz,
                                                    const f4 *nodes_q, uint32_t image_address, int repeat, int leaf_threshold, int busy_max,
                                                    uint32_t stack_limit) {
    int r_node = node_io;
    uint32_t r_sp = stack_top;
    unsigned long long all, inner, hl, hr, t, u;      /* lane masks (scalar register pairs the compiler picks) */
    int cnt, slow;
    /* v[32:35] = x lo, x hi, y lo, y hi; v[36:39] = z lo, z hi, left link, right link; v40 .. v45: the near / far dwords per axis */
#define NORI_QLOOP_FULL_CHECK "v_cmp_le_u32 vcc, %[limit], %[sp]\n\ts_cbranch_vccnz 4f\n\t"
#define NORI_QLOOP(FULL_CHECK) \
    asm volatile( \
        "s_mov_b64 %[all], exec\n\t" \
        "s_mov_b32 %[slow], 0\n\t" \
        "v_cmp_lt_i32 %[t], -1, %[node]\n"                        /* lanes at an inner node */ \
        "1:\n\t" \
        "s_and_b64 exec, %[all], %[t]\n\t" \
        "s_cbranch_execz 3f\n\t" \
        FULL_CHECK \
        /* fetch: the node's record from the LDS image (link carries kTopBit: quad offset in its low bits) or from memory */ \
        "v_cmp_lt_u32 vcc, 0x3fffffff, %[node]\n\t" \
        "s_mov_b64 %[inner], exec\n\t" \
        "s_and_b64 exec, %[inner], vcc\n\t" \
        "v_and_b32 v40, 0xffff, %[node]\n\t" \
        "v_lshl_add_u32 v40, v40, 4, %[image]\n\t" \
        "ds_read_b128 v[32:35], v40\n\t" \
        "ds_read_b128 v[36:39], v40 offset:16\n\t" \
        NORI_EXP_Q_LDS \
        "s_andn2_b64 exec, %[inner], vcc\n\t" \
        "s_cbranch_execz 2f\n\t" \
        "v_lshlrev_b32 v40, 5, %[node]\n\t"                       /* (other lanes than the ones that just used v40) */ \
        "global_load_dwordx4 v[32:35], v40, %[nodes]\n\t" \
        "global_load_dwordx4 v[36:39], v40, %[nodes] offset:16\n" \
        NORI_EXP_Q_GLOBAL \
        "2:\n\t" \
        "s_mov_b64 exec, %[inner]\n\t" \
        "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
        NORI_EXP_Q_ALU \
        /* per axis the dword with the near planes and the one with the far planes (mask = sign of the direction) */ \
        "v_bfi_b32 v40, %[mx], v33, v32\n\t" \
        "v_bfi_b32 v41, %[mx], v32, v33\n\t" \
        "v_bfi_b32 v42, %[my], v35, v34\n\t" \
        "v_bfi_b32 v43, %[my], v34, v35\n\t" \
        "v_bfi_b32 v44, %[mz], v37, v36\n\t" \
        "v_bfi_b32 v45, %[mz], v36, v37\n\t" \
        /* t = q A + (B -+ S) per plane, near = max over the axes, far = min; the dwords of the record are free by now. \
           (Both children of an axis in one v_pk_fma_f32 -- six packed instead of twelve plain multiply-adds -- measured 3.5 ms \
           per frame slower: the coefficients as register pairs cost the kernel a spill.) */ \
        NORI_SDWA("v32", "v40", "0") NORI_SDWA("v33", "v42", "0") NORI_SDWA("v34", "v44", "0") \
        "v_fma_f32 v32, v32, %[ax], %[bnx]\n\t" \
        "v_fma_f32 v33, v33, %[ay], %[bny]\n\t" \
        "v_fma_f32 v34, v34, %[az], %[bnz]\n\t" \
        "v_max3_f32 v32, v32, v33, v34\n\t"                       /* v32: near, left child */ \
        NORI_SDWA("v33", "v41", "0") NORI_SDWA("v34", "v43", "0") NORI_SDWA("v35", "v45", "0") \
        "v_fma_f32 v33, v33, %[ax], %[bfx]\n\t" \
        "v_fma_f32 v34, v34, %[ay], %[bfy]\n\t" \
        "v_fma_f32 v35, v35, %[az], %[bfz]\n\t" \
        "v_min3_f32 v33, v33, v34, v35\n\t"                       /* v33: far, left child */ \
        NORI_SDWA("v34", "v40", "1") NORI_SDWA("v35", "v42", "1") NORI_SDWA("v36", "v44", "1") \
        "v_fma_f32 v34, v34, %[ax], %[bnx]\n\t" \
        "v_fma_f32 v35, v35, %[ay], %[bny]\n\t" \
        "v_fma_f32 v36, v36, %[az], %[bnz]\n\t" \
        "v_max3_f32 v34, v34, v35, v36\n\t"                       /* v34: near, right child */ \
        NORI_SDWA("v35", "v41", "1") NORI_SDWA("v36", "v43", "1") NORI_SDWA("v37", "v45", "1") \
        "v_fma_f32 v35, v35, %[ax], %[bfx]\n\t" \
        "v_fma_f32 v36, v36, %[ay], %[bfy]\n\t" \
        "v_fma_f32 v37, v37, %[az], %[bfz]\n\t" \
        "v_min3_f32 v35, v35, v36, v37\n\t"                       /* v35: far, right child */ \
        "v_cmp_le_f32 vcc, v32, v33\n\t" \
        "v_cmp_le_f32 %[t], v32, %[tm]\n\t" \
        "v_cmp_le_f32 %[hl], 0, v33\n\t" \
        "v_cmp_le_f32 %[hr], v34, v35\n\t" \
        "v_cmp_le_f32 %[u], v34, %[tm]\n\t" \
        "s_and_b64 %[hl], %[hl], vcc\n\t" \
        "v_cmp_le_f32 vcc, 0, v35\n\t" \
        "s_and_b64 %[hl], %[hl], %[t]\n\t"                        /* left child hit */ \
        "s_and_b64 %[hr], %[hr], %[u]\n\t" \
        "s_and_b64 %[hr], %[hr], vcc\n\t"                         /* right child hit */ \
        /* selection: both -> the nearer one next, the other pushed; one -> that one; none -> pop.  "Left next" as a lane mask \
           (scalar unit): both and left nearer, or left alone */ \
        "v_cmp_le_f32 vcc, v32, v34\n\t" \
        "s_and_b64 %[t], %[hl], %[hr]\n\t"                        /* both */ \
        "s_or_b64 %[u], %[hl], %[hr]\n\t"                         /* any */ \
        "s_and_b64 vcc, vcc, %[t]\n\t" \
        "s_andn2_b64 %[hl], %[hl], %[hr]\n\t" \
        "s_or_b64 vcc, vcc, %[hl]\n\t" \
        "v_cndmask_b32 %[node], v39, v38, vcc\n\t"              /* the child walked next ... */ \
        "v_cndmask_b32 v40, v38, v39, vcc\n\t"                  /* ... and the other one */ \
        "s_mov_b64 exec, %[t]\n\t" \
        "ds_write_b32 %[sp], v40\n\t" \
        "v_add_u32 %[sp], %[stride], %[sp]\n\t" \
        "s_andn2_b64 exec, %[inner], %[u]\n\t" \
        "v_subrev_u32 %[sp], %[stride], %[sp]\n\t" \
        /* (the pop requested at the START of the step, with the node's record -- its link is dead by then -- so that no LDS trip ends \
           the step: bit-identical and no faster, headline 41.4 against 41.7 ms, profiles/r6_04_early_pop_ab.txt) */ \
        "ds_read_b32 %[node], %[sp]\n\t" \
        "s_mov_b64 exec, %[all]\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        /* again at once while enough lanes are at inner nodes -- or while some are and the trip around the loop outside would do \
           nothing else: no triangle step (too few lanes at a leaf) and no refill (too few idle lanes, or nothing to hand out) */ \
        "v_cmp_lt_i32 %[t], -1, %[node]\n\t" \
        "s_bcnt1_i32_b64 vcc_lo, %[t]\n\t" \
        "s_cmp_ge_u32 vcc_lo, %[repeat]\n\t" \
        "s_cbranch_scc1 1b\n\t" \
        "s_cmp_eq_u32 vcc_lo, 0\n\t" \
        "s_cbranch_scc1 3f\n\t" \
        "s_mov_b32 %[cnt], vcc_lo\n\t"                                /* lanes at inner nodes */ \
        "v_cmp_lt_u32 vcc, 0x80000000, %[node]\n\t"             /* lanes at a leaf */ \
        "s_bcnt1_i32_b64 vcc_lo, vcc\n\t" \
        "s_cmp_ge_u32 vcc_lo, %[leafth]\n\t" \
        "s_cbranch_scc1 3f\n\t" \
        "s_add_u32 vcc_lo, vcc_lo, %[cnt]\n\t"                        /* lanes with a ray in flight */ \
        "s_cmp_le_i32 vcc_lo, %[busymax]\n\t"                     /* idle lanes >= the refill threshold (and there is something to refill with) */ \
        "s_cbranch_scc0 1b\n" \
        "s_branch 3f\n" \
        "4:\n\t" \
        "s_mov_b32 %[slow], 1\n" \
        "3:\n\t" \
        "s_mov_b64 exec, %[all]\n\t" \
        : [node] "+v"(r_node), [sp] "+v"(r_sp), [all] "=&s"(all), [inner] "=&s"(inner), [hl] "=&s"(hl), [hr] "=&s"(hr), [t] "=&s"(t), [u] "=&s"(u), [cnt] "=&s"(cnt), [slow] "=&s"(slow) \
        : [tm] "v"(tmax), [ax] "v"(R.A[0]), [ay] "v"(R.A[1]), [az] "v"(R.A[2]), [bnx] "v"(R.Bn[0]), [bny] "v"(R.Bn[1]), [bnz] "v"(R.Bn[2]), \
          [bfx] "v"(R.Bf[0]), [bfy] "v"(R.Bf[1]), [bfz] "v"(R.Bf[2]), [mx] "v"(mx), [my] "v"(my), [mz] "v"(mz), \
          [nodes] "s"(nodes_q), [image] "s"(image_address), [repeat] "s"(repeat), [leafth] "s"(leaf_threshold), [busymax] "s"(busy_max), [limit] "s"(stack_limit), [stride] "n"(STACK_STRIDE) \
        : "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", \
          "vcc", "scc", "memory")
    if (CHECK_FULL) { NORI_QLOOP(NORI_QLOOP_FULL_CHECK); } else { NORI_QLOOP(""); }
#undef NORI_QLOOP
#undef NORI_QLOOP_FULL_CHECK
    node_io = r_node;
    stack_top = r_sp;
    return slow != 0;
}

/* hit_pack (wf_records.h) for wf_extend: the constants of "no closest hit" (t = inf, u = v = 0) are made from a zero the compiler
   cannot see through -- it otherwise keeps them as a register quad across the whole kernel, and with the register budget of 8 waves
   per SIMD that quad is what it spills (a scratch reload in front of every record store) */
__device__ __forceinline__ f4 hit_pack_here(const Hit *closest, bool shadow_occluded) {
    float z; asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    f4 h; h.x = u2f(0x7f800000u | f2u(z)); h.y = z; h.z = z;
    uint32_t w = kMissA;
    if (closest) { h.x = closest->t; h.y = closest->u; h.z = closest->v; if (closest->tri != kNoHit) w = closest->tri; }
    h.w = u2f(w | (shadow_occluded ? kOccludedB : 0u));
    return h;
}

/* Accel::rayIntersect for every path of copy `cur`: the shadow ray (if any) first, then the
   continuation ray, by the same lane; one 16-B hit record per path. */
/* BLOCK: threads per workgroup.  Every workgroup holds its own copy of the LDS image next to its stacks, so the bigger the
   workgroup the bigger the image can be: BVH2 trees run in workgroups of 1024 threads (two per CU: 2 x (68 KB of stacks +
   12 KB of image)), wide-node trees -- whose kernels need more than 64 registers, i.e. 5 or 6 waves per SIMD -- in workgroups of 256. */
template <int STACK, bool SPILL, bool COUNT, int MODE, bool WIDE, bool ASM, int BLOCK>
__global__ __launch_bounds__(BLOCK, WIDE ? (MODE != kStoredOnly ? 5 : 7) : 8) void wf_extend(DevScene sc, WfBuf b, int cur, int thresholds, WfBatch bt) {
    const int refill_threshold = thresholds & 0xff, leaf_threshold = (thresholds >> 8) & 0xff;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename ExtendStack<STACK, SPILL, ASM, BLOCK>::type Stack;
    Stack stack;
    stack.init(smem, b.stack_spill, gridDim.x * BLOCK);
    /* the first levels of the tree in LDS (rt_trace.h, node_fetch): behind the stacks */
    f4 *top = reinterpret_cast<f4 *>(smem + (size_t) Stack::kLdsEntries * BLOCK * sizeof(int));
    /* the kernel with the hand-written node loop walks the 32-B records: its image holds those (and so does the counting twin's) */
    const bool count_q = COUNT && !WIDE && (bt.flags & kBatchCountQ) != 0u;
    const int root_link = (ASM || count_q) ? top_image_to_lds(sc, top, sc.top_image_q, sc.top_image_q_quads) : top_image_to_lds(sc, top, sc.top_image, sc.top_image_quads);
    const TopNodesP top_lds = top_nodes_pointer(top);
    const uint32_t image_address = lds_address(smem) + (uint32_t) (Stack::kLdsEntries * BLOCK * sizeof(int));      /* of top */
    const WfState S = b.st[cur];
    static_assert(MODE == kStoredOnly || MODE == kFreshOnly, "wf_extend: stored paths and new paths are traced by separate launches");
    constexpr bool kFresh = MODE == kFreshOnly, kStored = MODE == kStoredOnly;
    const PassShape shape = pass_shape<MODE>(b.ctr, cur, bt);
    /* this launch's paths: the stored ones, indices [0, n_s), or the new ones, indices first + [0, n_fresh) */
    const uint32_t n = kFresh ? shape.n_fresh : shape.n_s, first = kFresh ? shape.n_f0 : 0u;
    /* the other copy's counters are free by now (its paths were consumed by the previous wf_shade):
       reset them for the wf_shade that follows this kernel and for the next wf_extend; the next pass starts its new camera
       samples where this one stops (a pass's stored-path launch passes the counter on unchanged, the launch of the new paths --
       behind it on the stream -- adds what it starts) */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        b.ctr[C_N + (cur ^ 1)] = 0u; b.ctr[C_HEAD + (cur ^ 1)] = 0u; b.ctr[C_HEAD_FRESH + (cur ^ 1)] = 0u;
        b.ctr[C_SAMPLE + (cur ^ 1)] = shape.s0 + shape.n_fresh;
    }
    const int lane = lane_id();
    Trav tv; trav_idle(tv);
    uint32_t rid = 0;            /* path << 2 | continuation pending << 1 | shadow ray occluded */
    bool unsaved = false;        /* the lane's last query is answered (tv.hit) but its record is not written yet */
    bool exhausted = n == 0;
    /* Paths are handed to waves in chunks: every wave starts with a static chunk (no atomic), the
       rest -- about half, for load balance -- is claimed dynamically with one atomic per chunk.  The
       chunk size follows the number of paths: big chunks amortise the atomic, small ones keep all
       waves busy; in the long tail of a batch the static chunks cover everything and no wave
       touches the counter (a single hot word sustains only ~90 atomics/us --
       MI355X_MICROARCH.md, row "dequeue" -- which used to cost 0.2 ms per tail iteration). */
    /* wave_id is the same in all lanes of a wave: readfirstlane tells the compiler, so the chunk cursor lives in SGPRs */
    const uint32_t n_waves = gridDim.x * (BLOCK / 64u), wave_id = (uint32_t) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6)));
    const uint32_t static_limit = (uint32_t) ((thresholds >> 16) & 0xfff) * n_waves;
    const uint32_t kChunk = n <= static_limit ? (((n + n_waves - 1u) / n_waves + 63u) & ~63u)      /* all static */
                                              : min(1024u, max(64u, (n / (n_waves * (uint32_t) ((thresholds >> 28) & 0xf))) & ~63u));
    const uint32_t dyn0 = n_waves * kChunk;        /* first dynamically claimed path */
    uint32_t chunk_pos = min(wave_id * kChunk, n), chunk_end = min(chunk_pos + kChunk, n);       /* wave-uniform */
    uint32_t nClosest = 0, nShadow = 0, nCam = 0;      /* wave-uniform: counted from ballots at the refill */
    uint32_t zc[Z_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};      /* wave-uniform census */
    TraversalCounters tc; tc.nodes = 0; tc.tris = 0;
    NORI_PROF_DECL
    while (true) {
        /* a lane is idle when it has no ray in flight: either it needs a new path, or its path's
           shadow ray is answered and the continuation ray is still to be traced (rid bit 1) */
        const bool pend = !trav_active(tv) && (rid & 2u) != 0u;
        const unsigned long long idle = __ballot(!trav_active(tv)), pending = __ballot(pend);
        const int nIdle = __popcll(idle);
        if ((!exhausted || pending != 0ull) && (nIdle >= refill_threshold || nIdle == 64)) {
            /* the wave owns [chunk_pos, chunk_end) and hands it out to its idle lanes */
            if (!exhausted && chunk_pos >= chunk_end) {
                uint32_t base = n;
                if (dyn0 < n) {
                    if (lane == 0) base = dyn0 + atomicAdd(&b.ctr[(kFresh ? C_HEAD_FRESH : C_HEAD) + cur], kChunk);
                    base = (uint32_t) __builtin_amdgcn_readfirstlane((int) base);
                }
                chunk_pos = base; chunk_end = min(base + kChunk, n);
                if (base >= n) { exhausted = true; chunk_pos = chunk_end = 0u; }
            }
            /* Results are written HERE, not in the trip a query ends: on average five lanes of a wave finish per trip,
               so storing right away ran the record packing at 5 / 64 lanes nearly every trip; at a refill >= 32 lanes are
               idle and write together.  An idle lane keeps its answer in tv.hit until then. */
            if (unsaved && !trav_active(tv)) {
                if (pend) rid |= tv.hit.tri != kNoHit ? 1u : 0u;      /* the shadow ray is answered; the continuation ray of the same vertex is next */
                else st_f4<1>(&b.hit[rid >> 2], tv.any ? hit_pack_here(nullptr, tv.hit.tri != kNoHit) : hit_pack_here(&tv.hit, (rid & 1u) != 0u));
                unsaved = false;
            }
            const unsigned long long fresh = idle & ~pending;
            if (COUNT) { zc[Z_REFILLS]++; zc[Z_REFILL_LANES] += (uint32_t) nIdle; }
            const uint32_t avail = chunk_end - chunk_pos;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (fresh >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) fresh, 0u));   /* set bits below this lane */
            bool startedA = false, startedB = false, startedCam = false;      /* this lane starts a closest-hit / a shadow query / a camera ray in this refill */
            const bool take = !pend && !trav_active(tv) && rank < avail;      /* this lane takes path chunk_pos + rank */
            if (kFresh && take) {      /* a new path: camera sample s0 + (i - n_f0) of the batch */
                const uint32_t i = first + chunk_pos + rank, sid = shape.s0 + chunk_pos + rank;
                f2 ps; RayIn ray; Rng rng;
                if (first_vertex(sc, bt, sid, ps, ray, rng)) {
                    st_f2<1>(&b.samp_pos[sid], ps);
                    rid = i << 2;
                    trav_begin<WIDE ? kLayoutWide : kLayoutBvh2>(sc, ray, false, stack, tv);
                    startedA = startedCam = true;
                    unsaved = trav_active(tv);
                    if (unsaved) tv.node = root_link;
                    if (!trav_active(tv)) st_f4<1>(&b.hit[i], hit_pack_here(nullptr, false));
                }
            } else if (kStored && (pend || take)) {
                const uint32_t i = pend ? (rid >> 2) : chunk_pos + rank;
                /* a fresh path: origin and both directions (the flags ride with the continuation direction) are requested
                   together -- one round trip to HBM instead of two (the direction a path needs first depends on its
                   flags).  A path whose shadow ray was just answered needs its continuation direction again (16 B; its
                   lane could not afford to keep it in registers during the shadow walk) -- the origin it still has. */
                f4 dB0; dB0.x = dB0.y = dB0.z = dB0.w = 0.0f;
                P3 o0; o0.x = tv.o.x; o0.y = tv.o.y; o0.z = tv.o.z;      /* a path whose shadow ray was just answered: the origin is still here */
                const f4 dA0 = S.dA[i];
                if (!pend) { o0 = S.o[i]; dB0 = S.dB[i]; }
                /* (the compiler sinks loads below the test of the flags -- a second trip to HBM per refill; naming them as inputs
                   of an empty asm statement pins all of them in front of it) */
                asm volatile("" :: "v"(o0.x), "v"(dA0.x), "v"(dB0.x));
                const uint32_t fl = pend ? F_HAS_A : state_flags(dA0);
                if (fl & (F_HAS_A | F_HAS_B)) {      /* 0: empty slot */
                    const bool any = (fl & F_HAS_B) != 0u;
                    const f4 d = any ? dB0 : dA0;
                    RayIn ray; ray.o = mk3(o0.x, o0.y, o0.z); ray.d = mk3(d.x, d.y, d.z);
                    ray.mint = kStoredMint; ray.maxt = any ? dB0.w : kInf;
                    rid = pend ? (rid & ~2u) : ((i << 2) | ((any && (fl & F_HAS_A)) ? 2u : 0u));
                    trav_begin<WIDE ? kLayoutWide : kLayoutBvh2>(sc, ray, any, stack, tv);
                    startedA = !any; startedB = any;
                    unsaved = trav_active(tv);
                    if (unsaved) tv.node = root_link;
                    if (!trav_active(tv)) {            /* empty scene: nothing occludes, nothing is hit */
                        if (rid & 2u) { startedA = true; rid &= ~2u; }      /* the continuation ray counts as traced, too */
                        st_f4<1>(&b.hit[i], hit_pack_here(nullptr, false));
                    }
                }
            }
            chunk_pos += min(avail, (uint32_t) __popcll(fresh));
            nClosest += (uint32_t) __popcll(__ballot(startedA));
            if (kFresh) nCam += (uint32_t) __popcll(__ballot(startedCam));
            if (kStored) nShadow += (uint32_t) __popcll(__ballot(startedB));
        }
        if (__ballot(trav_active(tv)) == 0ull) {
            if (exhausted && __ballot((rid & 2u) != 0u) == 0ull) break;
            continue;
        }
        NORI_PROF_MARK(prof_refill)
        /* inner-node steps run every trip, and again at once while enough lanes are at inner nodes (a tight loop without the
           refill test and the leaf vote: the trip's bookkeeping costs as much as a node step); the (rarer) triangle
           step only when enough lanes wait at a leaf or nobody has an inner node to test */
        if (COUNT) zc[Z_TRIPS]++;
        if constexpr (ASM) {
            static_assert(!WIDE && !COUNT, "the hand-written node loop: BVH2 nodes as 32-B records");
            /* the ray's plane coefficients (rt_nodeq.h), made anew for every pass through here: kept across the triangle step and
               the refill they would cost twelve registers the kernel does not have */
            f3 qo = tv.o, qr = tv.rcp;
            asm volatile("" : "+v"(qo.x), "+v"(qo.y), "+v"(qo.z), "+v"(qr.x), "+v"(qr.y), "+v"(qr.z));
            NodeqRay R;
            nodeq_ray(sc.grid, qo, qr, R);
            uint32_t stack_limit = 0xffffffffu;
            if constexpr (SPILL) stack_limit = stack.limit;
            const bool full = bvh2q_node_loop_asm<BLOCK * 4, SPILL>(tv.node, stack.top, tv.hit.t, R, (int) f2u(qr.x) >> 31, (int) f2u(qr.y) >> 31, (int) f2u(qr.z) >> 31,
                                           sc.nodes_q, image_address, bt.inner_repeat, leaf_threshold,
                                           /* lanes in flight at or below which the refill at the top of the loop would run: never (-1) if
                                              it has nothing to hand out */
                                           (!exhausted || __ballot((rid & 2u) != 0u) != 0ull) ? 64 - refill_threshold : -1, stack_limit);
            /* a lane's LDS stack is full (trees deeper than it): this step in C++, through the stack's global part */
            if (SPILL && full && trav_at_inner(tv)) trav_inner_step_q<false>(sc, stack, tv, tc, top_lds);
        } else
        do {
            if (COUNT) { const int ni = __popcll(__ballot(trav_at_inner(tv))); if (ni) { zc[Z_INNER_TRIPS]++; zc[Z_INNER_LANES] += (uint32_t) ni; } }
            if (trav_at_inner(tv)) {
                if (WIDE) trav_wide_step<COUNT>(sc, stack, tv, tc, top_lds);      /* BVH4, quantised boxes: scenes beyond the caches */
                else if (COUNT && count_q) trav_inner_step_q<COUNT>(sc, stack, tv, tc, top_lds);
                else trav_inner_step<COUNT>(sc, stack, tv, tc, top_lds);
            }
        } while (__popcll(__ballot(trav_at_inner(tv))) >= bt.inner_repeat);
        NORI_PROF_MARK(prof_node)
        const bool atLeaf = trav_at_leaf(tv);
        const int nLeaf = __popcll(__ballot(atLeaf));
        const bool innerLeft = __ballot(trav_at_inner(tv)) != 0ull;
        if (COUNT && nLeaf && (nLeaf >= leaf_threshold || !innerLeft)) { zc[Z_LEAF_TRIPS]++; zc[Z_LEAF_LANES] += (uint32_t) nLeaf; }
        if (atLeaf && (nLeaf >= leaf_threshold || !innerLeft)) trav_leaf_step<COUNT, false>(sc, stack, tv, tc, top_lds);
        NORI_PROF_MARK(prof_leaf)
    }
    /* the answers still held in registers when the wave ran out of paths (no lane is pending here: the loop ends only
       when no continuation ray is left): a path with a shadow ray only ends on it (tv.any); otherwise the closest hit
       + the shadow answer */
    if (unsaved) st_f4<1>(&b.hit[rid >> 2], tv.any ? hit_pack_here(nullptr, tv.hit.tri != kNoHit) : hit_pack_here(&tv.hit, (rid & 1u) != 0u));
    /* The ray counters: one atomic per WORKGROUP and counter.  One per wave -- 8192 waves x 2 - 3 atomics into one cache line, which takes
       ~90 of them per microsecond -- was a floor of ~0.18 ms under every launch whose waves end together: the small passes of a batch's tail,
       every pass of one device's share of eight.  The waves' stacks are free by now: the first words of the workgroup's LDS collect the sums. */
#ifdef NORI_LAB_WAVE_COUNTERS      /* A/B (variant builds): the counters per wave, as rounds 1 - 5 had them */
    if (lane == 0) {
        if (nClosest) atomicAdd(&b.stats[S_CLOSEST], (unsigned long long) nClosest);
        if (nShadow) atomicAdd(&b.stats[S_SHADOW], (unsigned long long) nShadow);
        if (kFresh && nCam) atomicAdd(&b.stats[S_CAM], (unsigned long long) nCam);
    }
#else
    __syncthreads();
    uint32_t *s_sum = reinterpret_cast<uint32_t *>(smem);
    if (threadIdx.x < 4u) s_sum[threadIdx.x] = 0u;
    __syncthreads();
    if (lane == 0) {
        if (nClosest) atomicAdd(&s_sum[0], nClosest);
        if (nShadow) atomicAdd(&s_sum[1], nShadow);
        if (kFresh && nCam) atomicAdd(&s_sum[2], nCam);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sum[0]) atomicAdd(&b.stats[S_CLOSEST], (unsigned long long) s_sum[0]);
        if (s_sum[1]) atomicAdd(&b.stats[S_SHADOW], (unsigned long long) s_sum[1]);
        if (kFresh && s_sum[2]) atomicAdd(&b.stats[S_CAM], (unsigned long long) s_sum[2]);
    }
#endif
    /* (counting builds: per wave, they are not timed) */
    if (COUNT) for (int off = 32; off > 0; off >>= 1) { tc.nodes += (uint32_t) __shfl_down((int) tc.nodes, off); tc.tris += (uint32_t) __shfl_down((int) tc.tris, off); }
    if (lane == 0) {
        if (COUNT) { atomicAdd(&b.stats[S_NODES], (unsigned long long) tc.nodes); atomicAdd(&b.stats[S_TRIS], (unsigned long long) tc.tris); }
        NORI_PROF_STORE
        if (COUNT && b.census) for (int k = 0; k < Z_COUNT; ++k) if (zc[k]) atomicAdd(&b.census[k], (unsigned long long) zc[k]);
    }
}


/* Tail overlap (wavefront_render): the records of a batch's last live paths move out of the state pool -- which the next batch
   is about to overwrite -- into the engine's side copy, where wf_finish walks them on its own CUs.
   (Compact records, wf_records.h: L lies at a 12-byte stride in the L_pdf allocation -- the first 16 n bytes copied here hold the 12 n
   in use; the rng array is idle and copied all the same.) */
__global__ __launch_bounds__(kB) void wf_tail_copy(WfBuf b, int cur, WfState D, uint32_t *d_ctr) {
    const WfState S = b.st[cur];
    const uint32_t n = b.ctr[C_N + cur];
    for (uint32_t i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB) {
        D.o[i] = S.o[i]; D.dA[i] = S.dA[i]; D.dB[i] = S.dB[i]; D.T_eta[i] = S.T_eta[i]; D.L_pdf[i] = S.L_pdf[i]; D.Ld[i] = S.Ld[i];
        D.sidx[i] = S.sidx[i]; D.rng[i] = S.rng[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { d_ctr[C_N] = n; d_ctr[C_TAIL_HEAD] = 0u; }
}

/* ----------------------------------------------------------- host driver */
constexpr int kShadeGridMax = 4096;

int shade_grid(size_t paths) { return (int) std::min<size_t>(kShadeGridMax, std::max<size_t>(64, (paths + kShadeChunk - 1) / kShadeChunk)); }

/* records per state copy for a batch of `paths`: the survivors plus the unused tail of every
   wf_shade workgroup's last chunk (a round that does not fit is split across two chunks, so
   nothing else is ever left empty) */
size_t state_capacity(size_t paths) {
    return paths + (size_t) kShadeChunk * (size_t) shade_grid(paths) * (size_t) (kB / kSB) + 1024;
}

struct Pool {
    std::vector<void *> allocs;
    size_t capacity = 0;       /* records per copy */
    size_t bytes = 0;
    WfBuf buf;
    uint32_t *h_ctr = nullptr; /* pinned */
    int *spill = nullptr;      /* traversal-stack overflow of wf_extend, one column per lane */
    size_t spill_ints = 0;
    void release() {
        for (void *p : allocs) (void) hipFree(p);
        allocs.clear(); capacity = 0; bytes = 0;
        if (spill) { (void) hipFree(spill); spill = nullptr; spill_ints = 0; }
        if (h_ctr) { (void) hipHostFree(h_ctr); h_ctr = nullptr; }
    }
};

#define WF_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__); } while (0)

template <class T> std::string pool_alloc(Pool &pool, T **out, size_t count) {
    void *p = nullptr;
    WF_TRY(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
    pool.allocs.push_back(p); pool.bytes += count * sizeof(T);
    *out = reinterpret_cast<T *>(p);
    return std::string();
}

/* bytes of path state per record: two copies of the SoA state + the hit record */
constexpr size_t kStateBytesPerRecord = 2 * (4 * sizeof(f4) + 2 * sizeof(P3) + sizeof(uint32_t) + sizeof(unsigned long long)) + sizeof(f4);

std::string ensure_pool(Pool &pool, size_t records) {
    if (pool.capacity >= records) return std::string();
    pool.release();
    WfBuf &b = pool.buf;
    std::string e;
#define A(field, count) if (!(e = pool_alloc(pool, &b.field, (count))).empty()) { pool.release(); return e; }
    for (int k = 0; k < 2; ++k) {
        A(st[k].o, records); A(st[k].dA, records); A(st[k].dB, records);
        A(st[k].T_eta, records); A(st[k].L_pdf, records); A(st[k].Ld, records);
        A(st[k].sidx, records); A(st[k].rng, records);
    }
    A(hit, records);
    A(ctr, (size_t) C_COUNT); A(stats, (size_t) S_COUNT);
#undef A
    WF_TRY(hipHostMalloc((void **) &pool.h_ctr, C_COUNT * sizeof(uint32_t)));
    pool.capacity = records;
    return std::string();
}

/* threads per wf_extend workgroup and workgroups per CU the LDS image is sized for, per node layout (see wf_extend) */
constexpr int kExtendBlockBvh2 = 1024, kExtendBlockWide = kB;
constexpr int kExtendWgsBvh2 = 2048 / kExtendBlockBvh2, kExtendWgsWide = 7, kExtendWgsWideFirst = 5;
constexpr size_t kLdsPerCu = 160 * 1024;
template <int STACK, bool SPILL, bool COUNT, int MODE>
void launch_extend(const DevScene &sc, const WfBuf &b, int cur, int refill, int grid, const WfBatch &bt, hipStream_t s) {
    const size_t image = (size_t) std::max(1u, sc.top_image_quads) * sizeof(f4);
    if (sc.wide) {
        /* wide trees push up to three children per step: always the spilling stack */
        const size_t lds = (size_t) LdsStackW<STACK, SPILL, kExtendBlockWide>::kLdsEntries * kExtendBlockWide * sizeof(int) + image;
        if (SPILL) hipLaunchKernelGGL((wf_extend<STACK, true, COUNT, MODE, true, false, kExtendBlockWide>), dim3(grid), dim3(kExtendBlockWide), lds, s, sc, b, cur, refill, bt);
    } else {
        /* the hand-written node loop (bvh2q_node_loop_asm) walks the tree's 32-B records (rt_nodeq.h: trees without unbounded boxes),
           addresses them by 32-bit byte offsets (trees below 2^25 nodes -- a BVH2 tree has fewer nodes than triangles) and keeps its
           stack in LDS; everything else takes the compiler's loop over the 64-B nodes */
        constexpr bool kAsm = !COUNT;
        const bool use_asm = kAsm && sc.nodes_q != nullptr && sc.n_triangles < (1u << 25) && (bt.flags & kBatchNoAsmLoop) == 0u;
        const bool image_q = use_asm || (COUNT && (bt.flags & kBatchCountQ) != 0u);
        const size_t lds = (use_asm ? (size_t) ExtendStack<STACK, SPILL, kAsm, kExtendBlockBvh2>::type::kLdsEntries : (size_t) LdsStackW<STACK, SPILL, kExtendBlockBvh2>::kLdsEntries) *
                               kExtendBlockBvh2 * sizeof(int) + (size_t) std::max(1u, image_q ? sc.top_image_q_quads : sc.top_image_quads) * sizeof(f4);
        if (use_asm)
            hipLaunchKernelGGL((wf_extend<STACK, SPILL, COUNT, MODE, false, kAsm, kExtendBlockBvh2>), dim3(grid), dim3(kExtendBlockBvh2), lds, s, sc, b, cur, refill, bt);
        else
            hipLaunchKernelGGL((wf_extend<STACK, SPILL, COUNT, MODE, false, false, kExtendBlockBvh2>), dim3(grid), dim3(kExtendBlockBvh2), lds, s, sc, b, cur, refill, bt);
    }
}

/* lds_stack: entries kept in LDS (16 / 24 / 32); spill: the tree is deeper than that;
   mode: kStoredOnly (the pass's stored paths) / kFreshOnly (its new ones) */
void launch_extend_dyn(const DevScene &sc, const WfBuf &b, int cur, int refill, int lds_stack, bool spill, bool count, int mode,
                       int grid, const WfBatch &bt, hipStream_t s) {
#define G(S, P, C) if (mode == kFreshOnly) launch_extend<S, P, C, kFreshOnly>(sc, b, cur, refill, grid, bt, s); \
                   else launch_extend<S, P, C, kStoredOnly>(sc, b, cur, refill, grid, bt, s)
#define E(S, P) if (count) { G(S, P, true); } else { G(S, P, false); }
#define F(S) if (spill) { E(S, true); } else { E(S, false); }
    if (lds_stack <= 16) { F(16); } else if (lds_stack <= 24) { F(24); } else { F(32); }
#undef F
#undef E
#undef G
}

/* Which record a render's paths are kept in (wf_records.h): the compact one where the scene is all-diffuse and the integrator one of
   path_mats / path_ems / path_mis -- the scenes whose wf_shade is the diffuse-only kernel, textured or not; every other scene, and
   every scene with NORI_HIP_WF_RECORD=full (read once per process), the full one and the kernels of before. */
bool record_compact(const DevScene &sc) {
    static const bool full = [] { const char *e = getenv("NORI_HIP_WF_RECORD"); return e && std::string(e) == "full"; }();
    if (sc.n_lights) return false;      /* delta lights: the general variants, on the full record (wavefront_lights.hip) */
    if (sc.env) return false;      /* an environment map: the one general variant, on the full record (wavefront_env.hip) */
    if (sc.medium.on) return false;      /* a medium: likewise (wavefront_medium.hip) */
    return !full && sc.integrator.type >= INT_MATS && sc.bsdf_mask == 1u && !getenv("NORI_HIP_SHADE_ANY_BSDF");
}

void launch_shade(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, int mode, int grid_, bool compact, hipStream_t s) {
    if (sc.gmed.rho && sc.integrator.type >= INT_MATS) { wf_grid_medium_launch_shade(sc, &b, cur, &bt, mode, grid_, s); return; }      /* kGridMedium: wavefront_grid_medium.hip */
    if (sc.n_lights && sc.integrator.type >= INT_EMS) { wf_lights_launch_shade(sc, &b, cur, &bt, mode, grid_, s); return; }      /* kDeltaLit: wavefront_lights.hip */
    if (sc.env && sc.integrator.type >= INT_MATS) { wf_env_launch_shade(sc, &b, cur, &bt, mode, grid_, s); return; }      /* kEnvLit: wavefront_env.hip */
    if (sc.medium.on && sc.integrator.type >= INT_MATS) { wf_medium_launch_shade(sc, &b, cur, &bt, mode, grid_, s); return; }      /* kMedium: wavefront_medium.hip */
    const dim3 grid(grid_ * (kB / kSB)), block(kSB);
    const bool lds_tables = shade_tables_fit(sc);
    /* the material set the kernel is compiled for: all-diffuse scenes (the Cornell box of the headline), scenes without a
       microfacet BSDF, any scene; integrators that never ask a BSDF (normals, ao, simple) have one kernel */
    int matset = sc.integrator.type < INT_WHITTED ? kAnyBsdf : sc.bsdf_mask == 1u ? 1 : (sc.bsdf_mask & 8u) == 0u ? 7 : kAnyBsdf;
    if (getenv("NORI_HIP_SHADE_ANY_BSDF")) matset = kAnyBsdf;      /* A/B: the general kernel whatever the scene holds */
    if (sc.integrator.type >= INT_WHITTED && sc.textured) matset = kAnyBsdf | kTextured;      /* textured albedos: one set, every BSDF */
    switch (sc.integrator.type) {
#define SH3(I, F, M) if (lds_tables) hipLaunchKernelGGL((wf_shade<I, F, true, M>), grid, block, 0, s, sc, b, cur, bt); \
                     else hipLaunchKernelGGL((wf_shade<I, F, false, M>), grid, block, 0, s, sc, b, cur, bt)
#define SH2(I, F) if (matset == 1) { SH3(I, F, 1); } else if (matset == 7) { SH3(I, F, 7); } else if (matset == kAnyBsdf) { SH3(I, F, kAnyBsdf); } \
                  else { SH3(I, F, kAnyBsdf | kTextured); }
#define SH1(I, F) SH3(I, F, kAnyBsdf)
        /* the compact record: the diffuse-only kernel, or the textured one (which an all-diffuse scene with textures runs) */
#define SH3C(I, F, M) if (lds_tables) hipLaunchKernelGGL((wf_shade_compact<I, F, true, M>), grid, block, 0, s, sc, b, cur, bt); \
                      else hipLaunchKernelGGL((wf_shade_compact<I, F, false, M>), grid, block, 0, s, sc, b, cur, bt)
#define SHC(I, F) if (!compact) { SH2(I, F); } else if (matset == 1) { SH3C(I, F, 1); } else { SH3C(I, F, kAnyBsdf | kTextured); }
#define SH(I, W) case I: if (mode == kFreshOnly) { W(I, kFreshOnly); } else if (mode == kMixed) { W(I, kMixed); } else { W(I, kStoredOnly); } break;
        SH(0, SH1) SH(1, SH1) SH(2, SH1) SH(3, SH2) SH(4, SHC) SH(5, SHC) SH(6, SHC)
#undef SH
#undef SHC
#undef SH3C
#undef SH1
#undef SH2
#undef SH3
    }
}

void launch_finish(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, bool count, int grid_, bool compact, hipStream_t s) {
    if (sc.gmed.rho && sc.integrator.type >= INT_MATS) { wf_grid_medium_launch_finish(sc, &b, cur, &bt, count, grid_, s); return; }
    if (sc.n_lights && sc.integrator.type >= INT_EMS) { wf_lights_launch_finish(sc, &b, cur, &bt, count, grid_, s); return; }
    if (sc.env && sc.integrator.type >= INT_MATS) { wf_env_launch_finish(sc, &b, cur, &bt, count, grid_, s); return; }
    if (sc.medium.on && sc.integrator.type >= INT_MATS) { wf_medium_launch_finish(sc, &b, cur, &bt, count, grid_, s); return; }
    const dim3 grid(grid_), block(kB);
    const size_t lds = (size_t) LdsStackW<16, true>::kLdsEntries * kB * sizeof(int);
    switch (sc.integrator.type) {
#define FN(I) case I: hipLaunchKernelGGL((wf_finish<I>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
#define FNT2(I, K) if (sc.textured) { hipLaunchKernelGGL((K<I, kAnyBsdf | kTextured>), grid, block, lds, s, sc, b, cur, bt, (int) count); } \
                   else { hipLaunchKernelGGL((K<I>), grid, block, lds, s, sc, b, cur, bt, (int) count); }
#define FNT(I) case I: FNT2(I, wf_finish) break;
#define FNC(I) case I: if (compact) { FNT2(I, wf_finish_compact) } else { FNT2(I, wf_finish) } break;
        FN(0) FN(1) FN(2) FNT(3) FNC(4) FNC(5) FNC(6)
#undef FNC
#undef FNT
#undef FNT2
#undef FN
    }
}

} // namespace

namespace nrt {

int wf_top_capacity(bool wide_nodes, bool records_32b, bool deeper_than_lds_stack) {
    /* 16 stack entries per lane in LDS, + 1: the "done" marker of the stacks that do not spill, + 1: the counter of the stack
       that spills behind the hand-written loop (LdsStackHybrid); the image in what is left */
    const size_t per_wg = kLdsPerCu / (wide_nodes ? kExtendWgsWide : kExtendWgsBvh2);
    const size_t stacks = (size_t) (deeper_than_lds_stack && records_32b ? 18 : 17) * (wide_nodes ? kExtendBlockWide : kExtendBlockBvh2) * sizeof(int);
    const int stride = records_32b ? kTopStrideQuadsQ : kTopStrideQuads;
    int n = 0;
    while (n < kTopMaxNodes && stacks + (size_t) top_image_quads(n + 1, stride) * sizeof(f4) <= per_wg) ++n;
    return n;
}


/* Everything a context keeps between render calls: the path-state pool, its streams and
   events, what the device offers.  One per nori_hip_ctx (= per GPU); nothing here is process-global,
   so contexts on different devices, or two contexts on one device, never share or free each
   other's buffers. */
/* Streams the engines are done with are PARKED, not destroyed, and the next engine on the same device that wants a stream of the
   same kind takes a parked one.  Why: with the HIP runtime this is built against, a hipMalloc that fails on a full device ends
   in a segmentation fault inside the runtime if streams with a CU mask that ran kernels with scratch memory were destroyed earlier
   in the process -- with project code or without (a 60-line program: create two masked streams, run a kernel with a private
   array on them, destroy them, fill the device, ask for more).  The same program survives when the streams are kept.  The
   out-of-memory retry of render_impl depends on that failure being an error code, and a process renders through many contexts.
   Parked streams are idle (synchronised before they are parked) and belong to nobody; one mutex guards the list. */
enum StreamKind { kStreamPlain = 0, kStreamTail = 1 };
struct ParkedStream { int device, kind, cus; hipStream_t stream; };
std::mutex g_parked_mutex;
std::vector<ParkedStream> g_parked;

void park_stream(int device, int kind, int cus, hipStream_t &st) {
    if (!st) return;
    (void) hipStreamSynchronize(st);
    std::lock_guard<std::mutex> lock(g_parked_mutex);
    g_parked.push_back(ParkedStream{device, kind, cus, st});
    st = nullptr;
}

hipStream_t unpark_stream(int device, int kind, int cus) {
    std::lock_guard<std::mutex> lock(g_parked_mutex);
    for (size_t i = 0; i < g_parked.size(); ++i)
        if (g_parked[i].device == device && g_parked[i].kind == kind && g_parked[i].cus == cus) {
            hipStream_t st = g_parked[i].stream;
            g_parked.erase(g_parked.begin() + (long) i);
            return st;
        }
    return nullptr;
}

struct WfEngine {
    int device = 0;                 /* the context's device: parked streams are handed out per device */
    Pool pool;
    hipStream_t stream = nullptr;   /* tail overlap: the bulk's (non-blocking; otherwise the bulk runs on the caller's stream) */
    hipEvent_t events[2] = {nullptr, nullptr};      /* tail overlap: the caller's work is queued / the bulk is done */
    int n_cus = 0;                  /* hipDeviceProp_t::multiProcessorCount of the context's device */
    /* tail overlap: the side copy of a batch's last live paths (wf_tail_copy), walked by wf_finish on tail_stream */
    struct TailSide {
        WfState st; uint32_t *ctr = nullptr; size_t capacity = 0; std::vector<void *> allocs;
        int *spill = nullptr; size_t spill_ints = 0;
        void release() { for (void *q : allocs) (void) hipFree(q); allocs.clear(); capacity = 0; ctr = nullptr; if (spill) { (void) hipFree(spill); spill = nullptr; spill_ints = 0; } }
    } tail;
    hipEvent_t tail_events[3] = {nullptr, nullptr, nullptr};      /* the side copy is filled / the tail is done / the tail is about to be dispatched */
    hipStream_t tail_stream = nullptr;
    int tail_stream_cus = 0;
    WfFirstLists *first = nullptr;      /* the per-tile candidate lists of the first pass (wavefront_first.hip), made when first needed */
};

/* The stream of the overlapped tails: it owns the CUs of the first `cus` mask bits.  The driver hands bit i of a queue's mask to
   XCD i mod 8 and walks an XCD's shader engines with the bits it gets, so 32 bits are one CU of every shader engine of every XCD:
   what is left for the other streams' kernels is even over XCDs (a kernel's workgroups go round the XCDs, b mod 8, whatever their
   CUs hold) and over the shader engines of an XCD (taking CUs from one shader engine only costs the bulk kernels twice the CUs'
   share -- pa5 table scene, bulk on the complement of 8 / 16 / 32 CUs of the FIRST shader engines: wf_extend +6 / +14 / +37 %,
   profiles/r5_07_tail_overlap_masks.txt). */
bool ensure_tail_stream(WfEngine &e, int cus) {
    if (e.tail_stream && e.tail_stream_cus == cus) return true;
    if (e.tail_stream) { park_stream(e.device, kStreamTail, e.tail_stream_cus, e.tail_stream); e.tail_stream_cus = 0; }
    if (cus < 8 || cus >= e.n_cus) return false;
    if ((e.tail_stream = unpark_stream(e.device, kStreamTail, cus)) != nullptr) { e.tail_stream_cus = cus; return true; }
    const uint32_t words = (uint32_t) ((e.n_cus + 31) / 32);
    std::vector<uint32_t> mask(words, 0u);
    for (int i = 0; i < cus; ++i) mask[(size_t) i / 32] |= 1u << (i % 32);
    if (hipExtStreamCreateWithCUMask(&e.tail_stream, words, mask.data()) != hipSuccess) { (void) hipGetLastError(); e.tail_stream = nullptr; return false; }
    e.tail_stream_cus = cus;
    return true;
}

std::string ensure_tail_side(WfEngine &e, size_t records, size_t spill_ints) {
    WfEngine::TailSide &t = e.tail;
    if (t.capacity < records) {
        t.release();
#define A(field, T) { void *q = nullptr; WF_TRY(hipMalloc(&q, records * sizeof(T))); t.allocs.push_back(q); t.st.field = reinterpret_cast<T *>(q); }
        A(o, P3) A(dA, f4) A(dB, f4) A(T_eta, f4) A(L_pdf, f4) A(Ld, P3) A(sidx, uint32_t) A(rng, unsigned long long)
#undef A
        { void *q = nullptr; WF_TRY(hipMalloc(&q, C_COUNT * sizeof(uint32_t))); t.allocs.push_back(q); t.ctr = reinterpret_cast<uint32_t *>(q); }
        t.capacity = records;
    }
    if (t.spill_ints < spill_ints) {
        if (t.spill) (void) hipFree(t.spill);
        t.spill = nullptr; t.spill_ints = 0;
        WF_TRY(hipMalloc((void **) &t.spill, spill_ints * sizeof(int)));
        t.spill_ints = spill_ints;
    }
    for (hipEvent_t &ev : e.tail_events) if (!ev) WF_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return std::string();
}

WfEngine *wavefront_create() {
    WfEngine *e = new WfEngine();
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) e->n_cus = prop.multiProcessorCount;
    e->device = dev;
    if (e->n_cus <= 0) e->n_cus = 256;
    return e;
}

void wavefront_destroy(WfEngine *e) {
    if (!e) return;
    e->pool.release();
    park_stream(e->device, kStreamPlain, 0, e->stream);
    for (hipEvent_t &ev : e->events) if (ev) { (void) hipEventDestroy(ev); ev = nullptr; }
    for (hipEvent_t &ev : e->tail_events) if (ev) { (void) hipEventDestroy(ev); ev = nullptr; }
    park_stream(e->device, kStreamTail, e->tail_stream_cus, e->tail_stream);
    e->tail.release();
    wf_first_destroy(e->first);
    delete e;
}

void wavefront_invalidate(WfEngine *e) { if (e) wf_first_invalidate(e->first); }

bool wavefront_excursions(unsigned long long out[4], bool reset) {
#if defined(NORI_COUNT_EXCURSIONS)
    unsigned long long h[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_nori_excursions), sizeof(h)) != hipSuccess) return false;
    for (int k = 0; k < 4; ++k) out[k] += h[k];
    if (reset) { const unsigned long long z[4] = {0, 0, 0, 0}; (void) hipMemcpyToSymbol(HIP_SYMBOL(g_nori_excursions), z, sizeof(z)); }
    return true;
#else
    (void) out; (void) reset;
    return false;
#endif
}

size_t wavefront_bytes_per_path() { return kStateBytesPerRecord; }
size_t wavefront_bytes_per_sample() { return 2 * (sizeof(f2) + sizeof(P3)); }      /* (two halves of the sample store: tail overlap) */
void wavefront_release_pool(WfEngine *e) { if (e) { e->pool.release(); e->tail.release(); } }

size_t wavefront_held_bytes(const WfEngine *e, const FilmStore &film) {
    return (e ? e->pool.bytes : 0) + film.capacity * (sizeof(f2) + sizeof(P3));
}

/* How a context launches wf_extend on a scene's tree -- what launch_extend_dyn and WfBatch are handed, the knobs of the environment
   included -- decided in ONE place for the two callers: a render's passes (wavefront_render) and the rays a caller brings itself
   (wavefront_trace), so that the second is held to the launch the first makes. */
struct ExtendPlan {
    int thresholds = 0;             /* refill | leaf << 8 | static paths per wave << 16 | dynamic divisor << 28 (wf_extend) */
    int lds_stack = 16;             /* traversal-stack entries kept in LDS */
    bool spill = false;             /* the tree needs more than that (or has wide nodes) */
    int extend_cus = 0;             /* CUs the persistent grid fills */
    int grid = 0, grid_first = 0;   /* workgroups: passes over stored paths / the launch of a pass's new paths */
    int inner_repeat = 24;
    uint32_t batch_flags = 0;       /* kBatchNoAsmLoop | kBatchCountQ */
    int finish_paths = 0, finish_grid = 0;      /* fewer live paths than this: wf_finish ends the batch; its grid */
    size_t spill_ints = 0;          /* of pool.spill, allocated here (0: no walk leaves the LDS stack) */
};

static std::string plan_extend(const WfEngine &eng, Pool &g_pool, const DevScene &sc, int stack_depth, bool count_traversal, ExtendPlan &plan) {
    int refill = 32;
    if (const char *e = getenv("NORI_HIP_WF_REFILL")) refill = std::min(64, std::max(1, atoi(e)));
    /* lanes at a leaf before a triangle step runs: 16 on BVH2 trees; 8 on wide trees, whose node steps are twice as long and whose
       waves hold fewer lanes per step (terrain, trace ms at 16 / 8 / 4: 54.2 / 53.3 / 53.2; the AO scene's BVH2 walk: 62.1 / 62.6 at 8;
       profiles/r4_05_sweeps.txt) */
    int leaf_th = sc.wide ? 8 : 16;
    if (const char *e = getenv("NORI_HIP_WF_LEAF")) leaf_th = std::min(64, std::max(1, atoi(e)));
    int static_per_wave = 1024, dyn_div = 8;      /* chunking of wf_extend: all-static below static_per_wave paths per wave, else n / (waves * dyn_div) per claim */
    if (const char *e = getenv("NORI_HIP_WF_STATIC")) static_per_wave = std::min(4095, std::max(0, atoi(e)));
    if (const char *e = getenv("NORI_HIP_WF_DYNDIV")) dyn_div = std::min(15, std::max(1, atoi(e)));
    plan.thresholds = refill | (leaf_th << 8) | (static_per_wave << 16) | (dyn_div << 28);
    /* traversal stack: what the tree needs, at most `lds_stack` entries of it in LDS */
    /* 16 entries in LDS, deeper walks spill to HBM: a stack of 24 entries costs three of the eight workgroups per CU, and walks
       rarely hold more than 16 deferred subtrees however deep the tree (measured, trace ms at 16 / 24 entries: table scene,
       depth 19: 77.5 / 83.0; Cornell box with the device builders' deeper trees: 61.6 / 74.8 and 73.3 / 82.1) */
    const bool no_asm_loop = getenv("NORI_HIP_WF_NO_ASM_LOOP") != nullptr && atoi(getenv("NORI_HIP_WF_NO_ASM_LOOP")) != 0;
    int lds_stack = 16;
    if (const char *e = getenv("NORI_HIP_WF_STACK")) lds_stack = atoi(e) <= 16 ? 16 : atoi(e) <= 24 ? 24 : 32;
    int finish_paths = 524288;           /* fewer live paths than this: wf_finish ends the batch */
    if (const char *e = getenv("NORI_HIP_WF_FINISH_PATHS")) finish_paths = std::max(256, atoi(e)) & ~255;
    const int finish_grid = finish_paths / kB;
    plan.finish_paths = finish_paths; plan.finish_grid = finish_grid;
    /* LDS per workgroup: stack entries (+1: the "done" marker of the non-spilling stack) + the top-node cache */
    const int extend_block = sc.wide ? kExtendBlockWide : kExtendBlockBvh2;
    /* which node loop wf_extend will run (launch_extend): the hand-written one on 32-B records, or the compiler's on 64-B nodes */
    const bool walk_q = !sc.wide && sc.nodes_q != nullptr && sc.n_triangles < (1u << 25) && !no_asm_loop;      /* 32-B node records */
    const bool node_loop_q = walk_q && !count_traversal;         /* ... by the hand-written loop */
    const bool count_q = walk_q && count_traversal;              /* ... by its C++ statement, counting (the same tree form as the timed kernel's) */
    bool spill = false;
    size_t lds_per_wg = 0;
    while (true) {
        spill = stack_depth > lds_stack || sc.wide != 0;
        const int stack_entries = node_loop_q ? lds_stack + (spill ? 2 : 1) : lds_stack + (spill ? 0 : 1);      /* kLdsEntries of the kernel's stack class */
        lds_per_wg = (size_t) stack_entries * extend_block * sizeof(int) + (size_t) std::max(1u, (node_loop_q || count_q) ? sc.top_image_q_quads : sc.top_image_quads) * sizeof(f4);
        /* the LDS image was sized at build_accel for 16-entry stacks (wf_top_capacity): a bigger stack asked for at render time
           (NORI_HIP_WF_STACK, an experiment knob) must not push a workgroup beyond its share of the CU's LDS -- fewer workgroups
           per CU than the kernel is built for, or a launch that fails: back to the stack the image was sized for */
        if (lds_stack > 16 && lds_per_wg > kLdsPerCu / (size_t) (sc.wide ? kExtendWgsWide : kExtendWgsBvh2)) { lds_stack = 16; continue; }
        break;
    }
    plan.lds_stack = lds_stack; plan.spill = spill;
    int per_cu = std::max(1, std::min(2048 / extend_block, (int) (kLdsPerCu / lds_per_wg)));      /* workgroups per CU */
    /* every workgroup of the persistent grid must be resident from the start (a workgroup that starts late owns a
       static share of the paths and works it off alone): the wide-node kernels are built for 7 waves per SIMD, their
       first-pass variant (camera rays computed in the kernel: 77 - 87 registers) for 5.  (Terrain, 10 M triangles, wf_extend ms per
       128 spp at 4 / 5 / 6 / 7 / 8 workgroups per CU: 65.7 / 57.8 / 53.9 / 53.6 / 54.2 -- the last two with the first pass still on the
       same grid; how many records the LDS image holds does not matter there: 113, 40 or none, profiles/r4_07_c5_occupancy.txt.) */
    if (sc.wide) per_cu = std::min(per_cu, kExtendWgsWide);
    if (const char *e = getenv("NORI_HIP_WF_EXTEND_WGS_PER_CU")) per_cu = std::min(2048 / extend_block, std::max(1, atoi(e)));
    const int extend_cus = eng.n_cus;      /* the persistent grid fills the device (a tail beside it: some of its workgroups start when
                                              the tail's have left -- handing them their first chunk in the order they start instead of
                                              by position was measured and is no faster, profiles/r5_11_tail_overlap_c4.txt) */
    plan.extend_cus = extend_cus;
    plan.grid_first = extend_cus * (sc.wide ? std::min(per_cu, kExtendWgsWideFirst) : per_cu);
    plan.grid = extend_cus * per_cu;
    plan.spill_ints = 0;
    if (stack_depth > 16) {      /* wf_finish keeps 16 entries in LDS */
        const size_t ints = (size_t) (stack_depth - 16) * std::max(plan.grid * extend_block, finish_grid * kB);
        if (g_pool.spill_ints < ints) {
            if (g_pool.spill) (void) hipFree(g_pool.spill);
            g_pool.spill = nullptr; g_pool.spill_ints = 0;
            WF_TRY(hipMalloc((void **) &g_pool.spill, ints * sizeof(int)));
            g_pool.spill_ints = ints;
        }
        plan.spill_ints = ints;
    }
    /* node steps repeat in a tight loop while >= 24 lanes of the wave are at inner nodes -- without the refill test, the leaf
       vote and the rest of the trip's bookkeeping, which cost as much as the node step itself (measured, wf_extend: Cornell
       box 51.7 -> 49.7 ms, 328 k-triangle AO 14.2 -> 12.8, table 77.7 -> 73.5, terrain 37.6 -> 34.7; the same loop
       around the triangle step compiles with 56 B of scratch and runs 50 % slower) */
    int inner_repeat = 24;
    if (const char *e = getenv("NORI_HIP_WF_INNER_REPEAT")) inner_repeat = std::min(65, std::max(1, atoi(e)));
    plan.inner_repeat = inner_repeat;
    plan.batch_flags = (no_asm_loop ? kBatchNoAsmLoop : 0u) | (count_q ? kBatchCountQ : 0u);
    return std::string();
}

std::string wavefront_render(WfEngine &eng, FilmStore &film_store, const DevScene &sc, const float *d_filter_table, const WfLaunch &L,
                             float *d_rgbw, void *stream_, WfStats &stats) {
    hipStream_t s = (hipStream_t) stream_;
    Pool &g_pool = eng.pool;
    stats = WfStats();
    if (L.n_sel_tiles == 0 || L.spp_count == 0) return std::string();

    /* a batch = a range of the call's tiles x as many samples per pixel as the film's sample store may hold
       (max_samples); the paths in flight -- the state pool -- are bounded separately (max_paths): a batch bigger than the pool
       starts its samples pass by pass, in the slots its finished paths leave (regeneration, WfBatch::pool) */
    const size_t budget = std::min<size_t>(std::max<size_t>(std::max(L.max_samples, L.max_paths), 256), (size_t) 1 << 31);
    uint32_t tiles_b = L.n_sel_tiles, spp_b = 1;      /* batch geometry */
    if ((size_t) L.n_sel_tiles * 256 > budget) tiles_b = (uint32_t) (budget / 256);
    else spp_b = (uint32_t) std::min<size_t>(L.spp_count, std::max<size_t>(1, budget / ((size_t) L.n_sel_tiles * 256)));
    const size_t batch_max = (size_t) tiles_b * 256 * spp_b;      /* camera samples of a batch */
    /* Tail overlap.  A batch ends with wf_finish walking its last <= finish_paths live paths to their ends: a launch as long as the
       batch's longest path (inside glass ~1300 vertices, one after the other) during which the device is next to idle -- 12 % of
       the pa5 table scene at 2048^2 x 1024 spp.  In a call of two or more batches the tail of batch k runs BESIDE the kernels of
       batch k + 1 instead: its records are copied out of the state pool (wf_tail_copy) and the persistent form of wf_finish walks
       them on a stream that owns `tail_cus` CUs (ensure_tail_stream) while the bulk of the next batch goes on on the engine's
       stream -- on the CUs the tail leaves it while it lasts (46 ms on 32 CUs), on all of them afterwards; the film gather of
       batch k -- which needs the tail's radiance -- is queued behind the bulk of batch k + 1.  The sample store has two halves,
       one per batch in flight.  Gathers stay in batch order, so the frame keeps its bits.  NORI_HIP_WF_TAIL_CUS (a multiple of 8;
       0: tails on the bulk's stream, as a call of one batch runs them). */
    int tail_cus = 32;
    if (const char *e = getenv("NORI_HIP_WF_TAIL_CUS")) tail_cus = std::max(0, atoi(e)) & ~7;
    const uint64_t batches = (uint64_t) ((L.n_sel_tiles + tiles_b - 1) / tiles_b) * ((L.spp_count + spp_b - 1) / spp_b);
    if (batches < 2 || L.film_reference || L.count_traversal || tail_cus >= eng.n_cus) tail_cus = 0;
    if (getenv("NORI_HIP_WF_FINISH") && atoi(getenv("NORI_HIP_WF_FINISH")) == 0) tail_cus = 0;
    if (tail_cus > 0 && !ensure_tail_stream(eng, tail_cus)) tail_cus = 0;
    const bool overlap = tail_cus > 0;
    if (L.film_reference && (tiles_b != L.n_sel_tiles || spp_b != L.spp_count || L.tile_mod != 1))
        return "wavefront: film_order = reference needs the whole frame in one batch (tile_mod 1, wavefront_samples >= pixels x samples)";
    size_t pool_paths = std::min(batch_max, std::max<size_t>(L.max_paths, 256));      /* paths in flight */
    if (const char *e = getenv("NORI_HIP_WF_POOL")) pool_paths = std::min(batch_max, (size_t) std::max(256ll, atoll(e)));      /* experiments */
    const size_t records = state_capacity(pool_paths);          /* per state copy */
    const int sh_grid = shade_grid(pool_paths);
    if (records >= ((size_t) 1 << 30)) return "wavefront: wavefront_paths too large (state index is 30 bits)";
    std::string err = ensure_pool(g_pool, records);
    if (!err.empty()) return err;
    FilmStore film;
    err = film_prepare(film_store, batch_max * (overlap ? 2 : 1), L.n_sel_tiles, L.tile_w, s, film);
    if (!err.empty()) return err;
    const bool moments = L.d_m2 != nullptr && L.moments != nullptr;
    if (moments) {
        err = film_moments_prepare(*L.moments, film, L.n_sel_tiles, L.tile_w, s);
        if (!err.empty()) return err;
    }
    stats.state_bytes = g_pool.bytes + batch_max * (overlap ? 2 : 1) * (sizeof(f2) + sizeof(P3));
    WF_TRY(hipMemsetAsync(g_pool.buf.stats, 0, S_COUNT * sizeof(unsigned long long), s));

    for (hipEvent_t &ev : eng.events) if (!ev) WF_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    /* the stream of the bulk -- everything but the overlapped tails: the caller's, or with overlap one of the engine's own (the
       caller's may be the legacy default stream, which runs nothing beside the work of another stream) */
    hipStream_t bulk = s;
    if (overlap) {
        if (!eng.stream) eng.stream = unpark_stream(eng.device, kStreamPlain, 0);
        if (!eng.stream) WF_TRY(hipStreamCreateWithFlags(&eng.stream, hipStreamNonBlocking));
        bulk = eng.stream;
    }
    WfBuf b = g_pool.buf;
    b.capacity = (uint32_t) records;
    b.samp_pos = film.pos; b.samp_L = film.L;
    uint32_t *const h_ctr = g_pool.h_ctr;
    hipStream_t tail_stream = overlap ? eng.tail_stream : nullptr;
    if (overlap) {      /* the bulk starts after whatever the caller queued on its stream */
        WF_TRY(hipEventRecord(eng.events[0], s));
        WF_TRY(hipStreamWaitEvent(bulk, eng.events[0], 0));
    }

    /* how wf_extend is launched on this scene (plan_extend: the knobs, the stack, the persistent grid, the spill buffer) */
    ExtendPlan plan;
    err = plan_extend(eng, g_pool, sc, L.stack_depth, L.count_traversal, plan);
    if (!err.empty()) return err;
    const int thresholds = plan.thresholds, lds_stack = plan.lds_stack, extend_cus = plan.extend_cus, extend_grid = plan.grid, extend_grid_first = plan.grid_first;
    const bool spill = plan.spill;
    const int finish_paths = plan.finish_paths, finish_grid = plan.finish_grid;
    if (plan.spill_ints != 0) b.stack_spill = g_pool.spill;
    stats.trace_cus = (uint32_t) extend_cus; stats.tail_cus = (uint32_t) tail_cus;
    const bool compact = record_compact(sc);
    stats.record = compact ? NORI_WF_RECORD_COMPACT : NORI_WF_RECORD_FULL;

    /* wf_finish: the persistent form (a lane pulls path after path) on four workgroups per CU of the stream it runs on -- the pa5
       table scene's tail 22 -> 19 ms on all CUs, 223 -> 80 ms on 16 (profiles/r5_06_tail_probe_c4.txt) */
    const int finish_grid_main = std::min(finish_grid, std::max(1, extend_cus * 4));
    const int finish_grid_side = std::min(finish_grid, std::max(1, tail_cus * 4));
    if (overlap) {
        err = ensure_tail_side(eng, (size_t) finish_paths, L.stack_depth > 16 ? (size_t) (L.stack_depth - 16) * finish_grid_side * kB : 0);
        if (!err.empty()) return err;
    }
    struct { bool active = false; FilmLaunch fl; FilmStore film; } pend;      /* overlap: the batch whose tail is in flight -- its film gather is still to come */

    int sync_every = 6;      /* path-loop iterations between two readbacks of the path count */
    if (const char *e = getenv("NORI_HIP_WF_SYNC_EVERY")) sync_every = std::min(64, std::max(1, atoi(e)));
    const bool census = getenv("NORI_HIP_CENSUS") != nullptr;
    bool use_finish = true;
    if (const char *e = getenv("NORI_HIP_WF_FINISH")) use_finish = atoi(e) != 0;
    const bool force_mixed = getenv("NORI_HIP_WF_FORCE_MIXED") != nullptr && atoi(getenv("NORI_HIP_WF_FORCE_MIXED")) != 0;      /* A/B, tests: every pass but the first as a pass that may hold new paths (both wf_extend launches, the kMixed wf_shade) */
    /* the new paths of a pass by per-tile candidate lists (wavefront_first.hip) where they apply: a pinhole, a BVH2 tree, no counting */
    bool first_lists = wf_first_applies(sc, L.count_traversal);
    if (first_lists) {
        if (!eng.first) eng.first = wf_first_create();
        WfFirstInfo fi;
        err = wf_first_prepare(*eng.first, sc, L.tiles_x, L.tiles_y, L.tile_w, s, fi);
        if (!err.empty()) return err;
        /* Worth it while few tiles overflow: a ray of an overflow tile walks the tree by the generic traverse<>, at several times the
           old kernel's cost per ray (headline: 4.4 times its average, a list tile 0.36).  Measured, share of the call's tiles on overflow:
           headline 2 % -2.0 ms; the pa5 table scene 7.6 % +12 ms (1 %) of its 1120; the AO icosphere 54 % +1.2 ms of 12.9
           (DESIGN.md section 7).  The lists run up to one tile in sixteen. */
        uint32_t sel_list = 0, sel_overflow = 0;      /* among the tiles this call renders */
        wf_first_selected(*eng.first, L.tile_mod, L.tile_rem, L.n_sel_tiles, L.tile_list != nullptr, sel_list, sel_overflow);
        if (!wf_first_forced() && (size_t) sel_overflow * 16 > (size_t) sel_list + sel_overflow) {
            first_lists = false;
            if (census) fprintf(stderr, "[wavefront first pass] walk (wf_extend): %u of %u tiles overflow at K %u\n", sel_overflow, sel_list + sel_overflow, fi.K);
        } else
        if (census) fprintf(stderr, "[wavefront first pass] lists: K %u, %u list tiles, %u overflow tiles, build %.3f ms (%s)\n", fi.K, fi.list_tiles, fi.overflow_tiles,
                            fi.build_ms, fi.rebuilt ? "built in this call" : "kept");
    } else if (census) fprintf(stderr, "[wavefront first pass] walk (wf_extend)\n");
    /* workgroups of 256 threads on the lanes the persistent grid of the first pass would take (and the spill buffer is sized for) */
    const int first_grid = extend_grid_first * (kExtendBlockBvh2 / kB);

    KernelTimer timer(L.time_kernels);
    unsigned long long *d_census = nullptr;
    if (census && L.count_traversal) {
        WF_TRY(hipMalloc((void **) &d_census, Z_COUNT * sizeof(unsigned long long)));
        WF_TRY(hipMemsetAsync(d_census, 0, Z_COUNT * sizeof(unsigned long long), s));
    }
    b.census = d_census;
    FilmLaunch fl;
    fl.tile_mod = L.tile_mod; fl.tile_rem = L.tile_rem; fl.tiles_x = L.tiles_x; fl.tiles_y = L.tiles_y; fl.tile_w = L.tile_w;
    fl.tile_list = L.tile_list; fl.tile_inverse = L.tile_inverse;

    /* one wf_extend launch of a pass: over its stored paths or over its new ones (pass_shape) */
    auto extend_pass = [&](int mode, const WfBatch &bt, int cur) -> std::string {
        timer.begin(KC_TRACE, bulk);
        if (mode == kFreshOnly && first_lists) wf_first_launch_extend(*eng.first, sc, &b, cur, &bt, first_grid, bulk);
        else launch_extend_dyn(sc, b, cur, thresholds, lds_stack, spill, L.count_traversal, mode, mode == kFreshOnly ? extend_grid_first : extend_grid, bt, bulk);
        WF_TRY(hipGetLastError());      /* a launch that did not fit (LDS, registers) must not pass for an empty pass */
        timer.end(bulk);
        stats.n_launches++;
        return std::string();
    };
    /* the film gather of the batch whose tail ran beside the current one: behind the tail, in front of everything that follows on
       the bulk's stream (gathers stay in batch order) */
    auto flush_pending = [&]() -> std::string {
        if (!pend.active) return std::string();
        WF_TRY(hipStreamWaitEvent(bulk, eng.tail_events[1], 0));
        timer.begin(KC_FILM, bulk);
        film_gather(sc, d_filter_table, pend.film, pend.fl, bulk);
        if (moments) film_gather_moments(sc, d_filter_table, pend.film, *L.moments, pend.fl, bulk);
        timer.end(bulk);
        stats.n_launches++;
        pend.active = false;
        return std::string();
    };

    /* the batches, one after the other: all samples of a range of tiles, range by range */
    WfBatch bt;
    bt.tile_mod = L.tile_mod; bt.tile_rem = L.tile_rem; bt.tiles_x = L.tiles_x; bt.tile_w = L.tile_w;
    bt.tile_list = L.tile_list;
    bt.inner_repeat = plan.inner_repeat;
    bt.flags = plan.batch_flags;
    bt.pool = (uint32_t) pool_paths;
    uint32_t t0 = 0, s0 = 0;      /* the next batch starts at this selected-tile ordinal and this sample of the call */
    while (t0 < L.n_sel_tiles) {
        bt.tile_first = t0; bt.n_tiles = std::min(tiles_b, L.n_sel_tiles - t0);
        bt.s_first = L.spp_begin + s0; bt.n_spp = std::min(spp_b, L.spp_count - s0);
        const uint32_t batch_samples = bt.n_tiles * 256u * bt.n_spp;
        const bool last_batch = s0 + bt.n_spp >= L.spp_count && t0 + bt.n_tiles >= L.n_sel_tiles;
        WF_TRY(hipMemsetAsync(b.ctr, 0, C_COUNT * sizeof(uint32_t), bulk));
        FilmStore bfilm = film;      /* the batch's part of the sample store */
        if (overlap) {      /* the sample store's halves alternate: the previous batch's tail and gather still use the other one */
            const size_t half = (size_t) (stats.n_batches & 1u) * batch_max;
            bfilm.pos += half; bfilm.L += half;
            b.samp_pos = bfilm.pos; b.samp_L = bfilm.L;
        }
        stats.n_batches++;
        int cur = 0, mode = kFreshOnly;      /* the state copy the next pass reads; the mode of its kernels */
        bool gather_deferred = false;
        /* rounds of passes until no path of the batch is alive.  A batch's paths die geometrically (Russian roulette from depth 3):
           thousands of rounds on ONE batch mean the loop is stuck; the bound is per batch, however many batches the call needs */
        uint32_t rounds = 0;
        while (true) {
            /* the path count is read back every sync_every iterations, more often once it is small
               (the readback costs ~20 us, an iteration on a few paths ~100 us) */
            const uint32_t n_max = mode != kStoredOnly ? 0xffffffffu : h_ctr[C_N + cur];
            const int iters = n_max > (16u << 20) ? sync_every : std::min(sync_every, 2);
            for (int it = 0; it < iters; ++it) {
                /* the pass's stored paths, then its new ones: two launches of the two pure kernels */
                if (mode != kFreshOnly && !(err = extend_pass(kStoredOnly, bt, cur)).empty()) return err;
                if (mode != kStoredOnly && !(err = extend_pass(kFreshOnly, bt, cur)).empty()) return err;
                timer.begin(KC_SHADE, bulk);
                launch_shade(sc, b, cur, bt, mode, sh_grid, compact, bulk);
                timer.end(bulk);
                /* the first pass started min(pool, samples) camera samples: a batch that fits the pool has none left */
                if (mode == kFreshOnly) mode = batch_samples <= bt.pool && !force_mixed ? kStoredOnly : kMixed;
                cur ^= 1;
                stats.n_launches++;
                stats.n_iterations++;
            }
            WF_TRY(hipMemcpyAsync(h_ctr, b.ctr, C_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, bulk));
            WF_TRY(hipStreamSynchronize(bulk));
            if (h_ctr[C_OVERFLOW] != 0) return "wavefront: path state pool overflow";
            /* camera samples of the batch no pass has started yet (the counter the next pass would read) */
            const uint32_t samples_left = batch_samples - std::min(batch_samples, h_ctr[C_SAMPLE + cur]);
            if (samples_left == 0u && mode == kMixed && !force_mixed) mode = kStoredOnly;
            if (census) fprintf(stderr, "[wavefront] iteration %u: %u path slots, %u samples to start\n", stats.n_iterations, h_ctr[C_N + cur], samples_left);
            if (samples_left == 0u && h_ctr[C_N + cur] != 0 && h_ctr[C_N + cur] <= (uint32_t) finish_paths && use_finish) {
                /* few live paths left: wf_finish walks them to their ends -- beside the next batch, or here */
                if (overlap && !last_batch) {
                    err = flush_pending();      /* (also: the previous tail is done with the side copy) */
                    if (!err.empty()) return err;
                    hipLaunchKernelGGL(wf_tail_copy, dim3(std::max(1u, (h_ctr[C_N + cur] + kB - 1) / kB)), dim3(kB), 0, bulk, b, cur, eng.tail.st, eng.tail.ctr);
                    WF_TRY(hipEventRecord(eng.tail_events[0], bulk));
                    WF_TRY(hipStreamWaitEvent(tail_stream, eng.tail_events[0], 0));
                    /* the bulk goes on once the tail is about to be dispatched: its workgroups take their CUs first */
                    WF_TRY(hipEventRecord(eng.tail_events[2], tail_stream));
                    WF_TRY(hipStreamWaitEvent(bulk, eng.tail_events[2], 0));
                    WfBuf tb = b;
                    tb.st[0] = eng.tail.st; tb.ctr = eng.tail.ctr; tb.stack_spill = eng.tail.spill; tb.capacity = (uint32_t) eng.tail.capacity;
                    timer.begin(KC_TAIL, tail_stream);
                    launch_finish(sc, tb, 0, bt, false, finish_grid_side, compact, tail_stream);
                    timer.end(tail_stream);
                    WF_TRY(hipEventRecord(eng.tail_events[1], tail_stream));
                    pend.active = true; pend.film = bfilm;
                    pend.fl = fl; pend.fl.tile_first = bt.tile_first; pend.fl.store_tile_first = bt.tile_first; pend.fl.n_tiles = bt.n_tiles; pend.fl.n_spp = bt.n_spp;
                    gather_deferred = true;
                    stats.n_launches += 2;
                } else {
                    timer.begin(KC_SHADE, bulk);
                    launch_finish(sc, b, cur, bt, L.count_traversal, finish_grid_main, compact, bulk);
                    timer.end(bulk);
                    stats.n_launches++;
                }
                break;
            }
            if (h_ctr[C_N + cur] == 0 && samples_left == 0u) break;
            if (++rounds > 20000) return "wavefront: path loop did not terminate";
        }
        /* batch done: splat its samples */
        if (!gather_deferred) {
            err = flush_pending();
            if (!err.empty()) return err;
            fl.tile_first = bt.tile_first; fl.store_tile_first = bt.tile_first; fl.n_tiles = bt.n_tiles; fl.n_spp = bt.n_spp;
            timer.begin(KC_FILM, bulk);
            if (!L.film_reference) film_gather(sc, d_filter_table, bfilm, fl, bulk);
            if (moments) film_gather_moments(sc, d_filter_table, bfilm, *L.moments, fl, bulk);
            timer.end(bulk);
            stats.n_launches++;
        }
        s0 += bt.n_spp;
        if (s0 >= L.spp_count) { s0 = 0; t0 += bt.n_tiles; }
    }
    if (overlap) {      /* back to the caller's stream */
        WF_TRY(hipEventRecord(eng.events[1], bulk));
        WF_TRY(hipStreamWaitEvent(s, eng.events[1], 0));
    }
    timer.begin(KC_FILM, s);
    if (L.film_reference) {
        err = film_reference_order(film_store, film, sc, d_filter_table, L.spp_count, L.tiles_x, L.film_share, d_rgbw, s);
        if (!err.empty()) return err;
    } else film_resolve(sc, film, fl, d_rgbw, s);
    if (moments) film_resolve_moments(sc, film, *L.moments, fl, L.d_m2, s);
    timer.end(s);
    stats.n_launches++;
    WF_TRY(hipGetLastError());
    unsigned long long h[S_COUNT];
    WF_TRY(hipMemcpyAsync(h, g_pool.buf.stats, sizeof(h), hipMemcpyDeviceToHost, s));
    WF_TRY(hipStreamSynchronize(s));
    stats.n_camera = h[S_CAM]; stats.n_closest = h[S_CLOSEST]; stats.n_shadow = h[S_SHADOW];
    stats.n_nodes = h[S_NODES]; stats.n_tris = h[S_TRIS];
    NORI_PROF_REPORT(h)
    stats.n_invalid = film_invalid_count(film, s);
    timer.collect(stats.class_ms, stats.class_launches);
    if (d_census) {
        unsigned long long z[Z_COUNT];
        WF_TRY(hipMemcpy(z, d_census, sizeof(z), hipMemcpyDeviceToHost));
        (void) hipFree(d_census);
        fprintf(stderr, "[wavefront census] trips %llu | node steps %llu, lanes/step %.1f | triangle steps %llu, lanes/step %.1f | refills %llu, idle lanes/refill %.1f\n",
                z[Z_TRIPS], z[Z_INNER_TRIPS], (double) z[Z_INNER_LANES] / std::max(1ull, z[Z_INNER_TRIPS]), z[Z_LEAF_TRIPS],
                (double) z[Z_LEAF_LANES] / std::max(1ull, z[Z_LEAF_TRIPS]), z[Z_REFILLS], (double) z[Z_REFILL_LANES] / std::max(1ull, z[Z_REFILLS]));
    }
    return std::string();
}

size_t wavefront_trace_max_rays(size_t max_paths) {
    /* a record's index is 30 bits of wf_extend's `rid`, and the pool holds state_capacity(n) records per copy */
    size_t n = std::min<size_t>(max_paths, (size_t) 1 << 29);
    while (n > 0 && state_capacity(n) >= ((size_t) 1 << 30)) n /= 2;
    return n;
}

std::string wavefront_trace(WfEngine &eng, const DevScene &sc, int stack_depth, bool count_traversal, const float *origins, const float *dir_a,
                            const float *dir_b, const uint32_t *flags, size_t n, float *hits, unsigned long long counts[4]) {
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (n == 0) return std::string();
    hipStream_t s = nullptr;
    Pool &pool = eng.pool;
    std::string err = ensure_pool(pool, state_capacity(n));
    if (!err.empty()) return err;
    ExtendPlan plan;
    err = plan_extend(eng, pool, sc, stack_depth, count_traversal, plan);
    if (!err.empty()) return err;
    WfBuf b = pool.buf;
    b.capacity = (uint32_t) pool.capacity;
    b.samp_pos = nullptr; b.samp_L = nullptr; b.census = nullptr;      /* (read by the launch of NEW paths and by counting builds under NORI_HIP_CENSUS only) */
    if (plan.spill_ints != 0) b.stack_spill = pool.spill;
    /* state copy 0 as wf_shade would have stored these paths (wf_records.h) */
    std::vector<P3> o(n); std::vector<f4> dA(n), dB(n);
    for (size_t i = 0; i < n; ++i) {
        o[i].x = origins[3 * i]; o[i].y = origins[3 * i + 1]; o[i].z = origins[3 * i + 2];
        f4 a; a.x = dir_a[3 * i]; a.y = dir_a[3 * i + 1]; a.z = dir_a[3 * i + 2]; a.w = kInf;
        dA[i] = state_dA(a, flags[i], (flags[i] & F_HAS_A) != 0u);
        dB[i].x = dir_b[4 * i]; dB[i].y = dir_b[4 * i + 1]; dB[i].z = dir_b[4 * i + 2]; dB[i].w = dir_b[4 * i + 3];
    }
    WF_TRY(hipMemcpy(b.st[0].o, o.data(), n * sizeof(P3), hipMemcpyHostToDevice));
    WF_TRY(hipMemcpy(b.st[0].dA, dA.data(), n * sizeof(f4), hipMemcpyHostToDevice));
    WF_TRY(hipMemcpy(b.st[0].dB, dB.data(), n * sizeof(f4), hipMemcpyHostToDevice));
    WF_TRY(hipMemsetAsync(b.hit, (int) (NORI_EXTEND_SENTINEL & 0xffu), n * sizeof(f4), s));
    uint32_t h_ctr[C_COUNT] = {0};
    h_ctr[C_N + 0] = (uint32_t) n;
    WF_TRY(hipMemcpy(b.ctr, h_ctr, sizeof(h_ctr), hipMemcpyHostToDevice));
    WF_TRY(hipMemsetAsync(pool.buf.stats, 0, S_COUNT * sizeof(unsigned long long), s));
    WfBatch bt;
    bt.tile_first = 0; bt.n_tiles = 0; bt.s_first = 0; bt.n_spp = 0; bt.tile_mod = 1; bt.tile_rem = 0; bt.tiles_x = 0; bt.tile_w = 0;
    bt.inner_repeat = plan.inner_repeat; bt.flags = plan.batch_flags; bt.pool = (uint32_t) n;
    launch_extend_dyn(sc, b, 0, plan.thresholds, plan.lds_stack, plan.spill, count_traversal, kStoredOnly, plan.grid, bt, s);
    WF_TRY(hipGetLastError());
    unsigned long long h[S_COUNT];
    WF_TRY(hipStreamSynchronize(s));
    WF_TRY(hipMemcpy(hits, b.hit, n * sizeof(f4), hipMemcpyDeviceToHost));
    WF_TRY(hipMemcpy(h, pool.buf.stats, sizeof(h), hipMemcpyDeviceToHost));
    counts[0] = h[S_CLOSEST]; counts[1] = h[S_SHADOW]; counts[2] = h[S_NODES]; counts[3] = h[S_TRIS];
    return std::string();
}

} // namespace nrt
