/*
 * wf_path_kernels.h -- wf_shade and wf_finish (wavefront.hip), the text of both kernels.  wavefront.hip includes it twice, inside its
 * unnamed namespace: once for the full path record (the kernels wf_shade / wf_finish) and once for the compact record of all-diffuse
 * scenes (wf_shade_compact / wf_finish_compact; wf_records.h).  Two kernels from one text, and not one body called by two kernels:
 * the full-record kernels then compile to the instructions and registers they had before the compact record existed.
 *     NORI_WF_SHADE_KERNEL, NORI_WF_FINISH_KERNEL    the kernels' names
 *     NORI_WF_KERNELS_COMPACT                        true / false
 */
template <int INTEG, int MODE, bool LDSTAB, int MATSET>
__global__ __launch_bounds__(kSB, NORI_SHADE_WGS) void NORI_WF_SHADE_KERNEL(DevScene sc, WfBuf b, int cur, WfBatch bt) {
    constexpr bool COMPACT = NORI_WF_KERNELS_COMPACT;
    NORI_LAB_SHADE_PAD
    static_assert(!COMPACT || INTEG >= INT_MATS, "the compact record: path_mats / path_ems / path_mis");
    constexpr int kLevel = COMPACT ? NORI_WF_COMPACT_LEVEL : 0;
    constexpr bool kDerive = kLevel >= 1, kNoEta = kLevel >= 2, kLsum = kLevel >= 3;
    const WfState S = b.st[cur], D = b.st[cur ^ 1];
    /* the compact record's radiance: three floats at a 12-byte stride in the L_pdf allocation */
    const P3 *S_L3 = reinterpret_cast<const P3 *>(S.L_pdf); P3 *D_L3 = reinterpret_cast<P3 *>(D.L_pdf);
    __shared__ unsigned long long s_skip[COMPACT ? 2 * kSkipDepths : 1];
    if (kDerive && MODE != kFreshOnly) skip_table_fill<INTEG>(s_skip);
    const uint32_t s_first = bt.s_first, n_spp = bt.n_spp;
    __shared__ uint4 s_tab[LDSTAB ? kShadeTabWords / 4 : 1];
    const typename ShadeTab<LDSTAB>::type tab = ShadeTab<LDSTAB>::make(sc, s_tab);      /* mesh / emitter tables: LDS instead of L2 round trips */
    constexpr bool kFresh = MODE != kStoredOnly, kStored = MODE != kFreshOnly;
    const PassShape shape = pass_shape<MODE>(b.ctr, cur, bt);      /* the pass wf_extend just traced: the same counters */
    const uint32_t n = shape.n, n_s = shape.n_s;
    const uint32_t rounds_total = (n + kSB - 1) / kSB;
    const uint32_t rounds_per_block = (rounds_total + gridDim.x - 1) / gridDim.x;
    const uint32_t r0 = blockIdx.x * rounds_per_block, r1 = min(rounds_total, r0 + rounds_per_block);
    /* rounds below r_mid hold stored paths, rounds from r_mid on new ones (pass_shape: the new paths start at a multiple of kSB) */
    const uint32_t r_mid = kStored ? min(r1, max(r0, shape.n_f0 / kSB)) : r0;
    __shared__ uint32_t s_wcnt[2][4], s_newbase;
    uint32_t out_base = 0u, out_used = 0u, out_len = 0u;     /* workgroup-uniform */
    bool overflow = false;
    const int wave = (int) (threadIdx.x >> 6), lane = lane_id();
    const uint32_t per_tile = 256u * n_spp;
    uint32_t pf_sidx = 0u; f4 pf_d, pf_L, pf_h;
    pf_d.x = pf_d.y = pf_d.z = pf_d.w = 0.0f; pf_L = pf_h = pf_d;
    /* One round: 256 paths, one vertex each.  FRESH rounds hold new paths -- camera sample s0 + (i - n_f0), nothing stored: the
       first vertex is recomputed from the sample index --, the others stored ones, whose record head was requested a round ahead.
       Two instantiations in two loops (a workgroup's range of rounds is stored rounds, then new ones): in ONE loop body the
       camera code and the prefetched head compete for registers and the kernel spills. */
    /* the head of a record, requested a round ahead (the radiance is part of it unless the shadow ray's answer decides where it is read: kLsum) */
#define NORI_SHADE_PREFETCH(k) \
    pf_d = ld_f4<2>(&S.dA[k]); pf_sidx = ld_w<2>(&S.sidx[k]); \
    if (!kNoEta) pf_L = ld_f4<2>(&S.L_pdf[k]); \
    else if (!kLsum) { const P3 l = ld_p3<2>(&S_L3[k]); pf_L.x = l.x; pf_L.y = l.y; pf_L.z = l.z; } \
    pf_h = ld_f4<1>(&b.hit[k]);
    auto round = [&](auto fresh_tag, uint32_t r, uint32_t r_end) {
        constexpr bool FRESH = decltype(fresh_tag)::value;
        const uint32_t i = r * kSB + threadIdx.x;
        bool survive = false;
        const uint32_t c_sidx = pf_sidx; const f4 c_d = pf_d, c_L = pf_L, c_h = pf_h;
        if (!FRESH && r + 1u < r_end && i + kSB < n_s) {
            NORI_SHADE_PREFETCH(i + kSB)
        }
        f4 n_o, n_dA, n_dB, n_T, n_L, n_Ld;
        uint32_t n_fl = 0u, sidx = 0u;
        unsigned long long n_rng = 0ull;
        if (FRESH ? i < n : i < n_s) {
            /* the path's state: from HBM, or -- first vertex -- recomputed from the sample index */
            uint32_t fl; f4 L4, d4, t4; Rng rng0; rng0.state = 0; rng0.inc = 0;
            f3 org = mk3(0.0f);      /* kMedium: the origin of the ray whose answer this vertex consumes (rt_path.h) */
            if (FRESH) {
                f2 ps; RayIn cam;
                sidx = shape.s0 + (i - shape.n_f0);
                fl = first_vertex(sc, bt, sidx, ps, cam, rng0) ? (F_HAS_A | (2u << 4)) : 0u;      /* prev_measure = discrete, depth 0 */
                L4.x = L4.y = L4.z = L4.w = 0.0f;                  /* L = 0, pdf_mat = 0 */
                t4.x = t4.y = t4.z = t4.w = 1.0f;                  /* T = 1, eta = 1 */
                d4.x = cam.d.x; d4.y = cam.d.y; d4.z = cam.d.z; d4.w = 0.0f;
                if (MATSET & kMedium) org = cam.o;
            } else {
                d4 = c_d;               /* the continuation direction and, in its w, the flags (wf_records.h) */
                fl = state_flags(d4);
            }
            if (fl & (F_HAS_A | F_HAS_B)) {
                if (!FRESH) { sidx = c_sidx; L4 = c_L; }
                const f4 h = FRESH ? ld_f4<1>(&b.hit[i]) : c_h;
                const uint32_t hw = __float_as_uint(h.w);
                bool done = false;
                NORI_LAB_SHADE_VERTEX
                if (kLsum && !FRESH) {                    /* path_on_shadow, done by the pass that stored the record: L, or L + Ld if unoccluded */
                    const bool lit = (fl & F_HAS_B) != 0u && !(hw & kOccludedB);
                    const P3 l = ld_p3<2>(lit ? &S.Ld[i] : &S_L3[i]);
                    L4.x = l.x; L4.y = l.y; L4.z = l.z;
                    if (fl & F_END_AFTER_B) done = true;
                } else
                if (fl & F_HAS_B) {                       /* path_on_shadow: add the emitter sample if unoccluded */
                    if (!(hw & kOccludedB)) {
                        const P3 ld = ld_p3<2>(&S.Ld[i]);
                        L4.x = L4.x + ld.x; L4.y = L4.y + ld.y; L4.z = L4.z + ld.z;
                    }
                    if (fl & F_END_AFTER_B) done = true;
                }
                PathState st;
                st.L = mk3(L4.x, L4.y, L4.z);
                if (!done) {
                    if (!FRESH) t4 = ld_f4<2>(&S.T_eta[i]);
                    Hit hit; bool found;
                    hit_unpack(sc, h, hit, found);
                    /* pcg32 stream of this camera sample: inc from the sample index, state from HBM */
                    const uint32_t sl = (sidx % per_tile) >> 8;
                    uint64_t rng_state = rng0.state;
                    if (!FRESH) rng_state = kDerive ? derived_rng_state<INTEG>(sc, bt, sidx, fl >> 8, s_skip) : ld_w<2>(&S.rng[i]);
                    if (kNoEta && !FRESH) vertex_unpack_diffuse(st, fl, p3_of(L4), t4, rng_state, ((uint64_t) (s_first + sl) << 1u) | 1u);
                    else
                    vertex_unpack(st, fl, L4, t4, rng_state, ((uint64_t) (s_first + sl) << 1u) | 1u);
                    if (MATSET & kMedium) {
                        if (!FRESH) { const P3 o3 = ld_p3<2>(&S.o[i]); org = mk3(o3.x, o3.y, o3.z); }
                        st.ray.o = org;
                    }
                    done = path_on_closest<INTEG, typename ShadeTab<LDSTAB>::type, MATSET>(sc, tab, st, hit, found, mk3(d4.x, d4.y, d4.z));
                    if (!done) {
                        survive = true;
                        if (kLsum) {
                            P3 l3, ls; ls.x = ls.y = ls.z = 0.0f;
                            vertex_pack_diffuse(st, n_o, n_dA, n_dB, n_T, l3, ls, n_fl);
                            n_L.x = l3.x; n_L.y = l3.y; n_L.z = l3.z; n_Ld.x = ls.x; n_Ld.y = ls.y; n_Ld.z = ls.z;
                        } else {
                            vertex_pack(st, n_o, n_dA, n_dB, n_T, n_L, n_Ld, n_fl);
                            if (kNoEta) n_T.w = n_L.w;
                        }
                        if (!kDerive) n_rng = st.rng.state;
                    }
                }
                if (done) {
                    P3 out; out.x = st.L.x; out.y = st.L.y; out.z = st.L.z;
                    st_p3<2>(&b.samp_L[sidx], out);
                }
            }
        }
        /* compaction: rank of this survivor among the workgroup's survivors of the round */
        const unsigned long long mask = __ballot(survive);
        if (lane == 0) s_wcnt[r & 1u][wave] = (uint32_t) __popcll(mask);
        shade_barrier();
        const uint32_t c0 = s_wcnt[r & 1u][0], c1 = kSB > 64 ? s_wcnt[r & 1u][1] : 0u, c2 = kSB > 128 ? s_wcnt[r & 1u][2] : 0u, c3 = kSB > 192 ? s_wcnt[r & 1u][3] : 0u;
        const uint32_t c = c0 + c1 + c2 + c3;
        uint32_t off = (uint32_t) __popcll(mask & ((1ull << lane) - 1ull));
        off += wave > 0 ? c0 : 0u; off += wave > 1 ? c1 : 0u; off += wave > 2 ? c2 : 0u;
        /* the round's survivors fill what is left of the current chunk, the rest opens a new one */
        const uint32_t room = out_len - out_used;
        uint32_t new_base = 0u, want = 0u;
        if (c > room) {                                  /* workgroup-uniform: reserve the next chunk */
            const uint32_t expect = c * (r1 - r);        /* survivors from here to the end of the range, at this round's rate */
            want = r + 1u == r1 ? c - room : min(kShadeChunk, max(c - room, ((expect + expect / 8u + 63u) & ~63u) - min(room, expect)));
            if (threadIdx.x == 0) s_newbase = atomicAdd(&b.ctr[C_N + (cur ^ 1)], want);
            shade_barrier();
            new_base = s_newbase;
            if (new_base + want > b.capacity) overflow = true;
        }
        if (survive && !overflow) {
            /* the record as it lies in HBM (wf_records.h): 100 B; the flags ride with the continuation direction, which is
               therefore always written */
            const uint32_t j = off < room ? out_base + out_used + off : new_base + (off - room);
            st_p3<2>(&D.o[j], p3_of(n_o)); st_f4<2>(&D.T_eta[j], n_T);
            if (kNoEta) st_p3<2>(&D_L3[j], p3_of(n_L)); else st_f4<2>(&D.L_pdf[j], n_L);
            st_f4<2>(&D.dA[j], state_dA(n_dA, n_fl, (n_fl & F_HAS_A) != 0u));
            if (!kDerive) st_w<2>(&D.rng[j], n_rng);
            st_w<2>(&D.sidx[j], sidx);
            if (n_fl & F_HAS_B) { st_f4<2>(&D.dB[j], n_dB); st_p3<2>(&D.Ld[j], p3_of(n_Ld)); }
            NORI_LAB_SHADE_STORE
        }
        if (c > room) { out_base = new_base; out_used = c - room; out_len = want; }
        else out_used += c;
    };
    if (kStored) {
        if (r0 < r_mid && r0 * kSB + threadIdx.x < n_s) {
            const uint32_t i0 = r0 * kSB + threadIdx.x;
            NORI_SHADE_PREFETCH(i0)
        }
        for (uint32_t r = r0; r < r_mid; ++r) round(std::false_type(), r, r_mid);
    }
    if (kFresh) for (uint32_t r = r_mid; r < r1; ++r) round(std::true_type(), r, r1);
    /* what is left of the last chunk holds no path: flags 0 */
    for (uint32_t k = out_used + threadIdx.x; k < out_len; k += kSB) { f4 z; z.x = z.y = z.z = z.w = 0.0f; D.dA[out_base + k] = z; }
    if (overflow && threadIdx.x == 0) b.ctr[C_OVERFLOW] = 1u;
}

#undef NORI_SHADE_PREFETCH

/* The long tail of a batch: once only a few thousand paths are alive, every wf_extend / wf_shade pair
   is a launch that lasts as long as ONE path vertex takes (~0.1 ms) however few paths there are.
   wf_finish ends it with one launch: each lane takes a path and walks it to its end -- shadow ray,
   continuation ray, Li vertex, repeat -- the megakernel's loop started from stored path state.
   (On a device of its own the launch lasts as long as the LONGEST path, ~1300 vertices through glass at p = 0.99, one after the
   other, however its lanes are used: a kernel that re-compacts a workgroup's paths after every vertex keeps the lanes dense and
   is no faster, profiles/r4_04_tail_per_vertex_ab.txt.  Nor does walking through
   the LDS image of the hot records help here -- pa5 table, 64 spp: 44.9 against 42.0 ms of shade time, a 1/8 share of the Cornell
   box 3.99 against 3.56: 2048 workgroups each copy 12 KB for a few hundred paths, and the C++ form of the 32-B node step pays 24
   instructions per step for the ray's plane coefficients.  Round 6, on the small persistent grid, through the image of the 64-B nodes:
   bit-identical and no faster either -- a path inside the glass sphere walks the BOTTOM of the tree --, profiles/r6_06_finish_image_ab.txt.) */
/* The lanes of a small persistent grid pull paths one by one -- a lane whose path has ended takes the next unclaimed one at the top
   of the vertex loop (one atomic per wave and refill), so a wave's lanes stay busy while paths are left and all of them are at the
   same stage of a vertex.  (Round 4's form -- one lane per path, a grid of finish_paths lanes -- ran at 6.5 of 64 lanes: pa5 table
   scene 22 -> 19 ms per tail on all CUs, 223 -> 80 ms on 16 CUs, where the tail of a batch runs when the NEXT batch runs beside it:
   what it costs there is CU time, not the length of the longest path.  profiles/r5_06_tail_probe_c4.txt.)  Same arithmetic per
   path, hence the same radiance; which lane walks a path is not observable. */
/* COMPACT: the records are compact ones (wf_records.h) -- a lane derives the pcg32 state once, when it takes a path, reads (T, pdf_mat)
   and the 12-B L, and from then on walks with live state as ever; the register that holds Ld holds Lsum = L + Ld instead, the record's
   or the lane's own. */
template <int INTEG, int MATSET = kAnyBsdf>      /* kAnyBsdf | kTextured: scenes with textured albedos (rt_path.h) */
__global__ __launch_bounds__(kB) void NORI_WF_FINISH_KERNEL(DevScene sc, WfBuf b, int cur, WfBatch bt, int count) {
    constexpr bool COMPACT = NORI_WF_KERNELS_COMPACT;
    static_assert(!COMPACT || INTEG >= INT_MATS, "the compact record: path_mats / path_ems / path_mis");
    constexpr int kLevel = COMPACT ? NORI_WF_COMPACT_LEVEL : 0;
    constexpr bool kDerive = kLevel >= 1, kNoEta = kLevel >= 2, kLsum = kLevel >= 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LdsStackW<16, true> stack;
    stack.init(smem, b.stack_spill, gridDim.x * kB);
    __shared__ uint4 s_tab[kShadeTabWords / 4];
    shade_tables_to_lds(sc, s_tab);
    const WfState S = b.st[cur];
    const uint32_t n = b.ctr[C_N + cur];
    const uint32_t per_tile = 256u * bt.n_spp;
    uint32_t nClosest = 0, nShadow = 0;
    TraversalCounters tc; tc.nodes = 0; tc.tris = 0;
    bool have = false, dry = false;      /* this lane walks a path / the paths have run out */
    uint32_t sidx = 0u, fl = 0u;
    f4 o, dA, dB, T, L, Ld;
    o.x = o.y = o.z = o.w = 0.0f; dA = dB = T = L = Ld = o;
    unsigned long long rng_state = 0ull;
    while (true) {
        const unsigned long long want = __ballot(!have && !dry);
        if (want != 0ull) {
            uint32_t base = 0u;
            if (lane_id() == 0) base = atomicAdd(&b.ctr[C_TAIL_HEAD], (uint32_t) __popcll(want));
            base = (uint32_t) __builtin_amdgcn_readfirstlane((int) base);
            const uint32_t i = base + __builtin_amdgcn_mbcnt_hi((uint32_t) (want >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) want, 0u));
            if (!have && !dry) {
                if (i >= n) dry = true;
                else {
                    dA = S.dA[i];
                    fl = state_flags(dA);
                    if (fl & (F_HAS_A | F_HAS_B)) {      /* (else: an empty slot -- the lane asks again in the next trip) */
                        have = true;
                        sidx = S.sidx[i]; dB = S.dB[i]; T = S.T_eta[i];
                        if (kNoEta) {      /* (T, pdf_mat), L at a 12-byte stride */
                            const P3 l = reinterpret_cast<const P3 *>(S.L_pdf)[i];
                            L.x = l.x; L.y = l.y; L.z = l.z; L.w = T.w; T.w = 1.0f;
                        } else L = S.L_pdf[i];
                        const P3 o3 = S.o[i], l3 = S.Ld[i];      /* (kLsum: Lsum) */
                        o.x = o3.x; o.y = o3.y; o.z = o3.z; o.w = kStoredMint; Ld.x = l3.x; Ld.y = l3.y; Ld.z = l3.z; Ld.w = 0.0f;
                        dA.w = kInf;
                        if (kDerive) rng_state = derived_rng_state<INTEG>(sc, bt, sidx, fl >> 8, nullptr);
                        else rng_state = S.rng[i];
                    }
                }
            }
        }
        if (__ballot(have) == 0ull) { if (__ballot(!dry) == 0ull) break; continue; }
        if (have) {      /* one vertex */
            bool fin = false;
            if (fl & F_HAS_B) {
                RayIn ray; ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(dB.x, dB.y, dB.z); ray.mint = kEpsilon; ray.maxt = dB.w;
                Hit sh; ++nShadow;
                if (!traverse<true>(sc, ray, true, stack, sh, tc)) {
                    if (kLsum) { L.x = Ld.x; L.y = Ld.y; L.z = Ld.z; }
                    else { L.x = L.x + Ld.x; L.y = L.y + Ld.y; L.z = L.z + Ld.z; }
                }
                fin = (fl & F_END_AFTER_B) != 0u;
            }
            if (!fin) {
                RayIn ray; ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(dA.x, dA.y, dA.z); ray.mint = o.w; ray.maxt = dA.w;
                Hit hit; ++nClosest;
                const bool found = traverse<true>(sc, ray, false, stack, hit, tc);
                if (found) hit.mesh = f2u(sc.shade_tris[(size_t) hit.tri * kShadeQuads].w);
                PathState st;
                vertex_unpack(st, fl, L, T, rng_state, ((uint64_t) (bt.s_first + ((sidx % per_tile) >> 8)) << 1u) | 1u);
                if (MATSET & kMedium) st.ray.o = ray.o;
                fin = path_on_closest<INTEG, MATSET>(sc, st, hit, found, ray.d);
                L.x = st.L.x; L.y = st.L.y; L.z = st.L.z;
                if (!fin) {
                    vertex_pack(st, o, dA, dB, T, L, Ld, fl); rng_state = st.rng.state;
                    if (kLsum && (fl & F_HAS_B)) { Ld.x = L.x + Ld.x; Ld.y = L.y + Ld.y; Ld.z = L.z + Ld.z; }
                }
            }
            if (fin) { P3 out; out.x = L.x; out.y = L.y; out.z = L.z; b.samp_L[sidx] = out; have = false; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        nClosest += (uint32_t) __shfl_down((int) nClosest, off);
        nShadow += (uint32_t) __shfl_down((int) nShadow, off);
        tc.nodes += (uint32_t) __shfl_down((int) tc.nodes, off); tc.tris += (uint32_t) __shfl_down((int) tc.tris, off);
    }
    /* one atomic per workgroup and counter (as wf_extend) */
    __shared__ uint32_t s_sum[4];
    __syncthreads();
    if (threadIdx.x < 4u) s_sum[threadIdx.x] = 0u;
    __syncthreads();
    if (lane_id() == 0) {
        if (nClosest) atomicAdd(&s_sum[0], nClosest);
        if (nShadow) atomicAdd(&s_sum[1], nShadow);
        if (count) { atomicAdd(&s_sum[2], tc.nodes); atomicAdd(&s_sum[3], tc.tris); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sum[0]) atomicAdd(&b.stats[S_CLOSEST], (unsigned long long) s_sum[0]);
        if (s_sum[1]) atomicAdd(&b.stats[S_SHADOW], (unsigned long long) s_sum[1]);
        if (count) { atomicAdd(&b.stats[S_NODES], (unsigned long long) s_sum[2]); atomicAdd(&b.stats[S_TRIS], (unsigned long long) s_sum[3]); }
    }
}
