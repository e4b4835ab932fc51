/*
 * harness.cpp -- TEST-ONLY: the compact path record of all-diffuse scenes (nori_amd/csrc/device/wf_records.h, rt_sampling.h) against
 * the full record, on the CPU, bit for bit.  A stand-alone program (tests/test_records_compact_cpu.py builds it with g++, once plain
 * and once with -fsanitize=address,undefined, and runs it as a process of its own):
 *
 *     harness closed-form                 rng_state_derived against rng_seed + n draws
 *     harness walk <scene file> <spp>     paths of every pixel of the scene, walked in lock step through vertex_pack / vertex_unpack
 *                                         with a carried pcg32 state and through vertex_pack_diffuse / vertex_unpack_diffuse with the
 *                                         derived state and Lsum -- the way wf_shade handles a stored vertex in either form
 *
 * The scene file is what the test writes from a tests/scenes.py scene: see read_scene.  Prints one line of counts; exit status 0 if
 * every comparison held, 1 with the first mismatches on stderr otherwise.
 */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nori_hip.h"
#include "../../nori_amd/csrc/device/wf_records.h"
#include "../../nori_amd/csrc/device/rt_path.h"
#include "../../nori_amd/csrc/device/scene_prep.h"
#include "../../nori_amd/csrc/device/film.h"      /* film_tile_pixel */

using namespace nrt;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "MISMATCH %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

constexpr uint32_t kTableDepths = 32u;      /* kSkipDepths of wavefront.hip: depths below it come from a table, the rest from the loop */

/* the skip pair the way the kernels get it: a table per integrator for the first depths, rng_skip_pair's loop beyond */
template <int INTEG> static RngSkip skip_for_depth(uint32_t depth) {
    static RngSkip table[kTableDepths];
    static bool filled = false;
    if (!filled) { for (uint32_t d = 0; d < kTableDepths; ++d) table[d] = rng_skip_pair(path_draws_diffuse<INTEG>(d)); filled = true; }
    return depth < kTableDepths ? table[depth] : rng_skip_pair(path_draws_diffuse<INTEG>(depth));
}

/* ------------------------------------------------------------------ closed form against drawing */
template <int INTEG> static uint64_t closed_form_cases() {
    const uint32_t depths[] = {0u, 1u, 2u, 3u, 4u, 5u, kTableDepths - 1u, kTableDepths, kTableDepths + 1u, 100u, 333u, 777u};
    /* pixel (width - 1, height - 1) of a 4096 x 4096 frame; streams s_first + sl near 2^31 */
    const uint64_t inits[] = {0ull, 1ull, 4095ull * 4096ull + 4095ull, 123456789ull, 45ull * 36ull + 44ull};
    const uint64_t seqs[] = {0ull, 1ull, 39ull, 0x7ffffff0ull, 0x7ffffffeull, 0x7fffffffull, 0x80000000ull, 0xffffffffull};
    uint64_t n_cases = 0;
    for (uint32_t d : depths) for (uint64_t init : inits) for (uint64_t seq : seqs) {
        const uint32_t n = path_draws_diffuse<INTEG>(d);
        /* the count itself, spelled out: camera sample, per vertex the BSDF pair (+ the emitter sample's four), roulette from depth 3 */
        uint32_t expect = 4u;
        for (uint32_t k = 0; k < d; ++k) expect += 2u + ((INTEG == INT_EMS || INTEG == INT_MIS) ? 4u : 0u) + (k >= 3u ? 1u : 0u);
        CHECK(n == expect, "integrator %d depth %u: %u draws, counted %u", INTEG, d, n, expect);
        Rng r; rng_seed(r, init, seq);
        for (uint32_t k = 0; k < n; ++k) (void) rng_next_uint(r);
        const RngSkip s = skip_for_depth<INTEG>(d);
        const uint64_t got = rng_state_derived(init, (seq << 1u) | 1u, s.A, s.G);
        CHECK(got == r.state, "integrator %d depth %u init %" PRIu64 " seq %" PRIu64 ": derived %016" PRIx64 ", drawn %016" PRIx64, INTEG, d, init, seq, got, r.state);
        CHECK(r.inc == ((seq << 1u) | 1u), "inc");
        /* and rng_advance from the seeded state, the library's own O(log n) form */
        Rng a; rng_seed(a, init, seq); rng_advance(a, n);
        CHECK(a.state == r.state, "rng_advance");
        ++n_cases;
    }
    return n_cases;
}

/* ------------------------------------------------------------------ scene */
struct ArrayStack {
    int data[128];
    int sp = 0;
    void reset() { sp = 0; }
    bool empty() const { return sp == 0; }
    int pop_or(int empty_value) { return sp == 0 ? empty_value : pop(); }
    void push(int v) { data[sp++] = v; }
    int pop() { return data[--sp]; }
};

struct SceneFile {
    std::vector<std::vector<float>> positions, normals;
    std::vector<std::vector<uint32_t>> indices;
    std::vector<nori_mesh_desc> meshes;
    nori_scene_desc desc;
};

template <class T> static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

/* magic "RCS1"; int32 integrator, width, height; float fov, near, far, to_world[16]; uint32 n_meshes; per mesh: uint32 n_vertices,
   n_triangles, has_normals; float albedo[3]; int32 is_emitter; float radiance[3]; positions; normals (if any); indices.
   Every BSDF is diffuse. */
static bool read_scene(const char *path, SceneFile &s) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char magic[4]; int32_t head[3]; float cam[19]; uint32_t n_meshes = 0;
    bool ok = rd(f, magic, 4) && memcmp(magic, "RCS1", 4) == 0 && rd(f, head, 3) && rd(f, cam, 19) && rd(f, &n_meshes, 1) && n_meshes <= 64;
    memset(&s.desc, 0, sizeof(s.desc));
    if (ok) {
        s.positions.resize(n_meshes); s.normals.resize(n_meshes); s.indices.resize(n_meshes); s.meshes.resize(n_meshes);
        for (uint32_t i = 0; ok && i < n_meshes; ++i) {
            uint32_t h[3]; float albedo[3], radiance[3]; int32_t emitter = 0;
            ok = rd(f, h, 3) && rd(f, albedo, 3) && rd(f, &emitter, 1) && rd(f, radiance, 3) && h[0] <= (1u << 20) && h[1] <= (1u << 20);
            if (!ok) break;
            s.positions[i].resize((size_t) 3 * h[0]); s.indices[i].resize((size_t) 3 * h[1]);
            ok = rd(f, s.positions[i].data(), s.positions[i].size());
            if (ok && h[2]) { s.normals[i].resize((size_t) 3 * h[0]); ok = rd(f, s.normals[i].data(), s.normals[i].size()); }
            ok = ok && rd(f, s.indices[i].data(), s.indices[i].size());
            for (uint32_t v : s.indices[i]) ok = ok && v < h[0];
            nori_mesh_desc &m = s.meshes[i];
            memset(&m, 0, sizeof(m));
            m.n_vertices = h[0]; m.n_triangles = h[1];
            m.positions = s.positions[i].data(); m.normals = h[2] ? s.normals[i].data() : nullptr; m.indices = s.indices[i].data();
            m.bsdf.type = 0; memcpy(m.bsdf.albedo, albedo, sizeof(albedo));
            m.bsdf.alpha = 0.1f; m.bsdf.int_ior = 1.5046f; m.bsdf.ext_ior = 1.000277f;
            m.is_emitter = emitter; memcpy(m.radiance, radiance, sizeof(radiance));
        }
    }
    fclose(f);
    if (!ok) return false;
    s.desc.n_meshes = n_meshes; s.desc.meshes = s.meshes.data();
    s.desc.camera.width = head[1]; s.desc.camera.height = head[2];
    s.desc.camera.fov = cam[0]; s.desc.camera.near_clip = cam[1]; s.desc.camera.far_clip = cam[2];
    memcpy(s.desc.camera.to_world, cam + 3, 16 * sizeof(float));
    s.desc.rfilter.type = 0; s.desc.rfilter.radius = 2.0f; s.desc.rfilter.stddev = 0.5f;
    s.desc.integrator.type = head[0];
    s.desc.sample_count = 1;
    return true;
}

struct Built {
    HostScene host; HostBvh bvh; DevScene dev;
};

static std::string build(const nori_scene_desc &desc, Built &b) {
    std::string err = prepare_scene(desc, b.host);
    if (err.empty()) err = build_bvh_sah(b.host, 64, b.bvh, false);
    if (!err.empty()) return err;
    DevScene &d = b.dev; HostScene &h = b.host;
    memset(&d, 0, sizeof(d));
    d.nodes = b.bvh.nodes.data(); d.tris = b.bvh.tris.data();
    d.positions = h.positions.data(); d.normals = h.normals.data(); d.texcoords = h.texcoords.data();
    d.indices = h.indices.data(); d.meshes = h.meshes.data(); d.emitter_cdf = h.emitter_cdf.data();
    d.emitters = h.emitters.data(); d.tri_mesh = h.tri_mesh.data();
    d.shade_tris = h.shade_tris.data();
    d.n_emitters = (uint32_t) h.emitters.size(); d.n_meshes = (uint32_t) h.meshes.size();
    d.n_triangles = (uint32_t) h.tri_mesh.size(); d.n_cdf = (uint32_t) h.emitter_cdf.size();
    d.root = b.bvh.root; d.wide = 0u;
    d.camera = h.camera; d.filter = h.filter; d.integrator = h.integrator;
    return std::string();
}

/* ------------------------------------------------------------------ lock-step walk */
static bool same(float a, float b) { return f2u(a) == f2u(b); }
static bool same3(const f3 &a, const f3 &b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
static bool same4(const f4 &a, const f4 &b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z) && same(a.w, b.w); }

struct WalkCounts {
    uint64_t paths = 0, stored = 0, past_table = 0, shadow = 0, lit = 0, end_after_b = 0, end_after_b_forced = 0;
    uint32_t max_depth = 0;
};

/* the state both forms must agree on after unpacking a vertex */
static void check_state(const PathState &a, const PathState &b, const char *where, uint32_t px, uint32_t py, uint32_t s) {
    CHECK(a.rng.state == b.rng.state && a.rng.inc == b.rng.inc, "%s pixel (%u, %u) sample %u depth %d: rng %016" PRIx64 " / %016" PRIx64, where, px, py, s, a.depth, a.rng.state, b.rng.state);
    CHECK(same3(a.T, b.T) && same3(a.L, b.L) && same(a.pdf_mat, b.pdf_mat) && same(a.eta, b.eta), "%s pixel (%u, %u) sample %u depth %d: T / L / pdf_mat / eta", where, px, py, s, a.depth);
    CHECK(a.depth == b.depth && a.prev_measure == b.prev_measure && a.phase == b.phase && a.end_after_shadow == b.end_after_shadow, "%s pixel (%u, %u) sample %u: depth / measure / phase", where, px, py, s);
}

/* What the next pass makes of a record with a shadow ray, in both forms: L (+ Ld if unoccluded) against the one of L / Lsum. */
static void check_shadow_step(const f4 &L, const f4 &Ld, const P3 &L3, const P3 &Lsum, bool occluded, const char *where) {
    f3 full = mk3(L.x, L.y, L.z);
    if (!occluded) { full.x = full.x + Ld.x; full.y = full.y + Ld.y; full.z = full.z + Ld.z; }
    const P3 &c = occluded ? L3 : Lsum;
    CHECK(same3(full, mk3(c.x, c.y, c.z)), "%s: radiance after the shadow ray (%s)", where, occluded ? "occluded" : "lit");
}

template <int INTEG>
static void walk_sample(const DevScene &sc, uint32_t px, uint32_t py, uint32_t s_first, uint32_t sl, WalkCounts &wc) {
    ArrayStack stack; TraversalCounters tc; tc.nodes = tc.tris = 0;
    /* first_vertex (wavefront.hip) */
    const uint64_t init = (uint64_t) py * (uint64_t) sc.camera.width + (uint64_t) px, inc = ((uint64_t) (s_first + sl) << 1u) | 1u;
    Rng rng0; rng_seed(rng0, init, (uint64_t) (s_first + sl));
    const f2 j = rng_next_2d(rng0);
    (void) rng_next_2d(rng0);
    RayIn cam; camera_sample_ray(sc.camera, mk2((float) px + j.x, (float) py + j.y), cam);
    CHECK(rng0.inc == inc, "inc");

    /* the record, full form (a: carried state) and compact form (b) */
    f4 o, dA, dB, T, L, Ld;
    o.x = cam.o.x; o.y = cam.o.y; o.z = cam.o.z; o.w = cam.mint;
    dA.x = cam.d.x; dA.y = cam.d.y; dA.z = cam.d.z; dA.w = cam.maxt;
    dB = dA; Ld.x = Ld.y = Ld.z = Ld.w = 0.0f;
    T.x = T.y = T.z = T.w = 1.0f; L.x = L.y = L.z = L.w = 0.0f;
    uint64_t rng_state = rng0.state;
    f4 T_pdf = T; P3 L3, Lsum; L3.x = L3.y = L3.z = 0.0f; Lsum = L3;
    uint32_t fl = F_HAS_A | (2u << 4);
    bool fresh = true;
    f3 end_a = mk3(0.0f), end_b = mk3(0.0f);
    ++wc.paths;
    while (true) {
        bool occluded = false;
        if (fl & F_HAS_B) {
            RayIn ray; ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(dB.x, dB.y, dB.z); ray.mint = kEpsilon; ray.maxt = dB.w;
            Hit sh; occluded = traverse<false>(sc, ray, true, stack, sh, tc);
            ++wc.shadow; if (!occluded) ++wc.lit;
        }
        f4 h;
        if (fl & F_HAS_A) {
            RayIn ray; ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(dA.x, dA.y, dA.z); ray.mint = o.w; ray.maxt = dA.w;
            Hit hit; (void) traverse<false>(sc, ray, false, stack, hit, tc);
            h = hit_pack(&hit, occluded);
        } else h = hit_pack(nullptr, occluded);
        /* wf_shade, full record: add the emitter sample if unoccluded */
        const bool lit = (fl & F_HAS_B) && !(f2u(h.w) & kOccludedB);
        if (lit) { L.x = L.x + Ld.x; L.y = L.y + Ld.y; L.z = L.z + Ld.z; }
        /* wf_shade, compact record: ONE of L / Lsum (a new path has L = 0) */
        P3 Lc = lit ? Lsum : L3;
        if (fresh) { Lc.x = Lc.y = Lc.z = 0.0f; }
        CHECK(same3(mk3(L.x, L.y, L.z), mk3(Lc.x, Lc.y, Lc.z)), "pixel (%u, %u) sample %u: L after the shadow ray", px, py, sl);
        end_a = mk3(L.x, L.y, L.z); end_b = mk3(Lc.x, Lc.y, Lc.z);
        if (fl & F_END_AFTER_B) { ++wc.end_after_b; break; }
        Hit hit; bool found;
        hit_unpack(sc, h, hit, found);
        PathState a, b;
        vertex_unpack(a, fl, L, T, rng_state, inc);
        if (fresh) {
            f4 one, zero; one.x = one.y = one.z = one.w = 1.0f; zero.x = zero.y = zero.z = zero.w = 0.0f;
            vertex_unpack(b, fl, zero, one, rng0.state, inc);
        } else {
            const uint32_t depth = fl >> 8;
            const RngSkip k = skip_for_depth<INTEG>(depth);
            vertex_unpack_diffuse(b, fl, Lc, T_pdf, rng_state_derived(init, inc, k.A, k.G), inc);
            ++wc.stored;
            if (depth >= kTableDepths) ++wc.past_table;
            if (depth > wc.max_depth) wc.max_depth = depth;
        }
        check_state(a, b, "unpacked", px, py, sl);
        const f3 d = mk3(dA.x, dA.y, dA.z);
        const bool done_a = path_on_closest<INTEG>(sc, a, hit, found, d), done_b = path_on_closest<INTEG>(sc, b, hit, found, d);
        CHECK(done_a == done_b, "pixel (%u, %u) sample %u: one form ends, the other goes on", px, py, sl);
        end_a = a.L; end_b = b.L;
        if (done_a || done_b) break;
        check_state(a, b, "shaded", px, py, sl);
        f4 o2, dA2, dB2; uint32_t fl2 = 0u;
        dA2.x = dA2.y = dA2.z = dA2.w = 0.0f; dB2 = dA2; dB = dA2;
        vertex_pack(a, o, dA, dB, T, L, Ld, fl);
        vertex_pack_diffuse(b, o2, dA2, dB2, T_pdf, L3, Lsum, fl2);
        rng_state = a.rng.state;
        CHECK(fl == fl2 && same4(o, o2), "pixel (%u, %u) sample %u: flags %08x / %08x or origin", px, py, sl, fl, fl2);
        if (fl & F_HAS_A) CHECK(same4(dA, dA2), "pixel (%u, %u) sample %u: continuation ray", px, py, sl);
        if (fl & F_HAS_B) CHECK(same4(dB, dB2), "pixel (%u, %u) sample %u: shadow ray", px, py, sl);
        CHECK(same(T.x, T_pdf.x) && same(T.y, T_pdf.y) && same(T.z, T_pdf.z) && same(L.w, T_pdf.w) && same(T.w, 1.0f), "pixel (%u, %u) sample %u: T / pdf_mat / eta", px, py, sl);
        CHECK(same3(mk3(L.x, L.y, L.z), mk3(L3.x, L3.y, L3.z)), "pixel (%u, %u) sample %u: L", px, py, sl);
        if (fl & F_HAS_B) {
            check_shadow_step(L, Ld, L3, Lsum, false, "stored record"); check_shadow_step(L, Ld, L3, Lsum, true, "stored record");
            /* A path that ends after its shadow ray: diffuse BSDFs alone never make one (bsdf_sample and bsdf_eval vanish together), so
               the record of this vertex is packed once more with end_after_shadow set, in both forms, and taken through the pass that
               would consume it. */
            PathState ea = a, eb = b; ea.end_after_shadow = eb.end_after_shadow = 1;
            f4 eo; eo.x = eo.y = eo.z = eo.w = 0.0f;
            f4 edA = eo, edB = eo, eT = eo, eL = eo, eLd = eo, eo2 = eo, edA2 = eo, edB2 = eo, eTp = eo; uint32_t efl = 0u, efl2 = 0u;
            P3 eL3, eLsum; eL3.x = eL3.y = eL3.z = 0.0f; eLsum = eL3;
            vertex_pack(ea, eo, edA, edB, eT, eL, eLd, efl);
            vertex_pack_diffuse(eb, eo2, edA2, edB2, eTp, eL3, eLsum, efl2);
            CHECK(efl == efl2 && (efl & F_END_AFTER_B) && !(efl & F_HAS_A) && same4(edB, edB2) && same4(eo, eo2), "forced end after the shadow ray: flags / rays");
            check_shadow_step(eL, eLd, eL3, eLsum, false, "forced end after the shadow ray"); check_shadow_step(eL, eLd, eL3, eLsum, true, "forced end after the shadow ray");
            ++wc.end_after_b_forced;
        }
        /* through HBM (wf_records.h): origin and emitter sample as three floats, flags in the continuation direction's w */
        { const f4 stored = state_dA(dA, fl, (fl & F_HAS_A) != 0u); const P3 o3 = p3_of(o), l3 = p3_of(Ld);
          fl = state_flags(stored); dA = stored; dA.w = kInf;
          o.x = o3.x; o.y = o3.y; o.z = o3.z; o.w = kStoredMint; Ld.x = l3.x; Ld.y = l3.y; Ld.z = l3.z; Ld.w = 0.0f; }
        fresh = false;
    }
    CHECK(same3(end_a, end_b), "pixel (%u, %u) sample %u: radiance (%g %g %g) / (%g %g %g)", px, py, sl, end_a.x, end_a.y, end_a.z, end_b.x, end_b.y, end_b.z);
}

template <int INTEG> static void walk(const DevScene &sc, uint32_t s_first, uint32_t spp, WalkCounts &wc) {
    for (uint32_t py = 0; py < (uint32_t) sc.camera.height; ++py)
        for (uint32_t px = 0; px < (uint32_t) sc.camera.width; ++px)
            for (uint32_t s = 0; s < spp; ++s) walk_sample<INTEG>(sc, px, py, s_first, s, wc);
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "closed-form") {
        const uint64_t n = closed_form_cases<INT_MATS>() + closed_form_cases<INT_EMS>() + closed_form_cases<INT_MIS>();
        printf("closed-form cases %" PRIu64 " failures %d\n", n, g_failures);
        return g_failures ? 1 : 0;
    }
    if (argc >= 4 && std::string(argv[1]) == "walk") {
        SceneFile sf; Built b;
        if (!read_scene(argv[2], sf)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        const std::string err = build(sf.desc, b);
        if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
        const uint32_t spp = (uint32_t) atoi(argv[3]), s_first = argc >= 5 ? (uint32_t) strtoul(argv[4], nullptr, 10) : 0u;
        WalkCounts wc;
        switch (b.dev.integrator.type) {
        case INT_MATS: walk<INT_MATS>(b.dev, s_first, spp, wc); break;
        case INT_EMS: walk<INT_EMS>(b.dev, s_first, spp, wc); break;
        case INT_MIS: walk<INT_MIS>(b.dev, s_first, spp, wc); break;
        default: fprintf(stderr, "the compact record: path_mats / path_ems / path_mis\n"); return 2;
        }
        printf("walk paths %" PRIu64 " stored %" PRIu64 " past_table %" PRIu64 " max_depth %u shadow %" PRIu64 " lit %" PRIu64 " end_after_b %" PRIu64 " forced %" PRIu64 " failures %d\n",
               wc.paths, wc.stored, wc.past_table, wc.max_depth, wc.shadow, wc.lit, wc.end_after_b, wc.end_after_b_forced, g_failures);
        return g_failures ? 1 : 0;
    }
    fprintf(stderr, "usage: %s closed-form | walk <scene file> <spp> [first sample]\n", argv[0]);
    return 2;
}
