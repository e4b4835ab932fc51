/*
 * harness.cpp -- TEST-ONLY: the per-tile candidate lists of the first pass (nori_amd/csrc/device/first_lists.h) on the CPU.
 * tests/test_first_lists_cpu.py builds it with g++ into a shared library of its own and calls it through ctypes.
 *
 *   fl_create     prepare_scene + a tree: the host's SAH builder (0) or the device builders' steps run as loops (1: PLOC, radius 8,
 *                 the tree a context builds by default; tests/emu/emu_builder.h)
 *   fl_lists      first_camera / first_tile_frustum / first_tile_walk for every tile of the frame: counts and lists
 *   fl_tiles_on_big_meshes   which tiles see a mesh of many triangles (where the overflow tiles must lie)
 *   fl_check      camera rays of every tile that has a list -- the extreme jitters (0 and the largest float below 1, both axes) of
 *                 the tile's four corner pixels and `per_pixel` seeded samples of every pixel, drawn as first_vertex draws them --
 *                 through the walk of rt_trace.h (traverse<>) and, every `scan_every`-th ray, through the linear scan of all pair
 *                 records; the hit triangle must be in the tile's list and first_list_trace must return the same (t, u, v, tri),
 *                 bit for bit
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nori_hip.h"
#include "../emu/emu_builder.h"
#include "../../nori_amd/csrc/device/rt_path.h"
#include "../../nori_amd/csrc/device/scene_prep.h"
#include "../../nori_amd/csrc/device/film.h"      /* film_tile_pixel */
#include "../../nori_amd/csrc/device/first_lists.h"

using namespace nrt;

struct ArrayStack {
    int data[128];
    int sp = 0;
    void reset() { sp = 0; }
    int pop_or(int empty_value) { return sp == 0 ? empty_value : data[--sp]; }
    void push(int v) { data[sp++] = v; }
};

struct fl_ctx {
    HostScene host; HostBvh bvh; DevScene dev;
};

extern "C" {

int fl_create(const nori_scene_desc *scene, int builder, fl_ctx **out) {
    fl_ctx *c = new fl_ctx();
    std::string err = prepare_scene(*scene, c->host);
    if (err.empty()) {
        if (builder == 1) { EmuBuilderStats st; err = build_bvh_steps_host(c->host, false, 8u, c->bvh, &st); }
        else err = build_bvh_sah(c->host, 64, c->bvh, false);
    }
    if (!err.empty()) { fprintf(stderr, "fl_create: %s\n", err.c_str()); delete c; return 1; }
    DevScene &d = c->dev; HostScene &h = c->host;
    memset(&d, 0, sizeof(d));
    d.nodes = c->bvh.nodes.data(); d.tris = c->bvh.tris.data();
    d.positions = h.positions.data(); d.normals = h.normals.data(); d.texcoords = h.texcoords.data();
    d.indices = h.indices.data(); d.meshes = h.meshes.data(); d.tri_mesh = h.tri_mesh.data(); d.shade_tris = h.shade_tris.data();
    d.n_meshes = (uint32_t) h.meshes.size(); d.n_triangles = (uint32_t) h.tri_mesh.size();
    d.root = c->bvh.root; d.wide = 0u;
    d.camera = h.camera; d.filter = h.filter; d.integrator = h.integrator;
    *out = c;
    return 0;
}
void fl_destroy(fl_ctx *c) { delete c; }

/* info = {n_nodes, n_pairs, root link, max depth} */
void fl_info(const fl_ctx *c, int64_t info[4]) {
    info[0] = c->bvh.n_nodes; info[1] = c->bvh.n_pairs; info[2] = c->dev.root; info[3] = c->bvh.max_depth;
}

/* margin[3] = {theta, eps_z, pad_abs} of the tile at (x0, y0), ok flags in the return value (bit 0 camera, bit 1 pyramid) */
int fl_margin(const fl_ctx *c, int x0, int y0, double margin[3]) {
    FirstCamera C; first_camera(c->dev, C);
    FirstFrustum F; first_tile_frustum(c->dev.camera, C, x0, y0, 1.0, F);
    margin[0] = F.theta; margin[1] = F.eps_z; margin[2] = C.pad_abs;
    return (C.ok ? 1 : 0) | (F.ok ? 2 : 0);
}

static void tiles_of(const DevScene &sc, uint32_t &tx, uint32_t &ty) {
    tx = (uint32_t) (sc.camera.width + kTile - 1) / kTile; ty = (uint32_t) (sc.camera.height + kTile - 1) / kTile;
}

/* count[tile], pairs[tile][K]; returns the number of tiles */
uint32_t fl_lists(const fl_ctx *c, uint32_t K, double margin_scale, uint32_t *count, uint32_t *pairs) {
    const DevScene &sc = c->dev;
    uint32_t tx, ty; tiles_of(sc, tx, ty);
    if (K > kFirstListMaxK) return 0;
    FirstCamera C; first_camera(sc, C);
    for (uint32_t tile = 0; tile < tx * ty; ++tile) {
        FirstFrustum F; first_tile_frustum(sc.camera, C, (int) (tile % tx) * kTile, (int) (tile / tx) * kTile, margin_scale, F);
        uint32_t local[kFirstListMaxK];
        const uint32_t n = first_tile_walk(sc, C, F, margin_scale, K, local);
        count[tile] = n;
        if (n != kFirstListOverflow) for (uint32_t k = 0; k < n; ++k) pairs[(size_t) tile * K + k] = local[k];
    }
    return tx * ty;
}

/* out[tile] = 1 iff the ray through the centre of some pixel of the tile hits a mesh of at least min_tris triangles (the walk) */
void fl_tiles_on_big_meshes(const fl_ctx *c, uint32_t min_tris, uint8_t *out) {
    const DevScene &sc = c->dev;
    uint32_t tx, ty; tiles_of(sc, tx, ty);
    ArrayStack stack; TraversalCounters tc; tc.nodes = tc.tris = 0;
    for (uint32_t tile = 0; tile < tx * ty; ++tile) {
        out[tile] = 0;
        for (int pix = 0; pix < 256 && !out[tile]; ++pix) {
            const int px = (int) (tile % tx) * kTile + (pix & 15), py = (int) (tile / tx) * kTile + (pix >> 4);
            if (px >= sc.camera.width || py >= sc.camera.height) continue;
            RayIn ray; camera_sample_ray(sc.camera, mk2((float) px + 0.5f, (float) py + 0.5f), ray);
            Hit hit; traverse<false>(sc, ray, false, stack, hit, tc);
            if (hit.tri != kNoHit && sc.meshes[sc.tri_mesh[hit.tri]].n_triangles >= min_tris) out[tile] = 1;
        }
    }
}

static bool same_bits(float a, float b) { return f2u(a) == f2u(b); }

/* out = {rays, hits, rays scanned, hit triangle not in the list, list trace != walk, scan != walk, list tiles, overflow tiles} */
int fl_check(const fl_ctx *c, uint32_t K, double margin_scale, uint32_t per_pixel, uint32_t scan_every, uint64_t out[8]) {
    const DevScene &sc = c->dev;
    uint32_t tx, ty; tiles_of(sc, tx, ty);
    const uint32_t n_tiles = tx * ty;
    std::vector<uint32_t> count(n_tiles), pairs((size_t) n_tiles * std::max(1u, K));
    if (fl_lists(c, K, margin_scale, count.data(), pairs.data()) != n_tiles) return 1;
    const uint32_t n_pairs = c->bvh.n_pairs;
    const int W = sc.camera.width, H = sc.camera.height;
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::vector<uint64_t>> acc(nt, std::vector<uint64_t>(8, 0));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t] {
        uint64_t *a = acc[t].data();
        ArrayStack stack; TraversalCounters tc; tc.nodes = tc.tris = 0;
        uint64_t serial = 0;
        auto one = [&](uint32_t tile, f2 ps) {
            RayIn ray; camera_sample_ray(sc.camera, ps, ray);
            Hit walk; traverse<false>(sc, ray, false, stack, walk, tc);
            const uint32_t *list = pairs.data() + (size_t) tile * std::max(1u, K);
            Hit got; first_list_trace(sc, ray, list, count[tile], got);
            a[0]++;
            if (walk.tri != kNoHit) {
                a[1]++;
                bool in_list = false;
                for (uint32_t k = 0; k < count[tile] && !in_list; ++k) {
                    const f4 q4 = sc.tris[(size_t) list[k] * kPairQuads + 4];
                    in_list = f2u(q4.z) == walk.tri || f2u(q4.w) == walk.tri;
                }
                if (!in_list) { if (a[3]++ < 5) fprintf(stderr, "tile %u ps (%.9g, %.9g): hit triangle %u is not in the list\n", tile, ps.x, ps.y, walk.tri); }
            }
            if (!(got.tri == walk.tri && same_bits(got.t, walk.t) && same_bits(got.u, walk.u) && same_bits(got.v, walk.v))) {
                if (a[4]++ < 5) fprintf(stderr, "tile %u ps (%.9g, %.9g): list (%u, %.9g) walk (%u, %.9g)\n", tile, ps.x, ps.y, got.tri, got.t, walk.tri, walk.t);
            }
            if (scan_every && (serial++ % scan_every) == 0) {      /* the linear scan: every pair record, in order */
                Hit scan; scan.tri = kNoHit; scan.mesh = kNoHit; scan.t = ray.maxt; scan.u = scan.v = 0.0f;
                for (uint32_t p = 0; p < n_pairs; ++p) {
                    const f4 *tq = sc.tris + (size_t) p * kPairQuads;
                    first_pair_step(tq[0], tq[1], tq[2], tq[3], tq[4], ray.o, ray.d, ray.mint, scan);
                }
                a[2]++;
                if (!(scan.tri == walk.tri && same_bits(scan.t, walk.t) && same_bits(scan.u, walk.u) && same_bits(scan.v, walk.v))) a[5]++;
            }
        };
        const float below_one = u2f(0x3f7fffffu);
        for (uint32_t tile = t; tile < n_tiles; tile += nt) {
            if (count[tile] == kFirstListOverflow) { a[7]++; continue; }
            a[6]++;
            const int x0 = (int) (tile % tx) * kTile, y0 = (int) (tile / tx) * kTile;
            const int x1 = std::min(x0 + kTile, W) - 1, y1 = std::min(y0 + kTile, H) - 1;
            const int cx[2] = {x0, x1}, cy[2] = {y0, y1};
            for (int ix = 0; ix < 2; ++ix) for (int iy = 0; iy < 2; ++iy)
                for (int jx = 0; jx < 2; ++jx) for (int jy = 0; jy < 2; ++jy)
                    one(tile, mk2((float) cx[ix] + (jx ? below_one : 0.0f), (float) cy[iy] + (jy ? below_one : 0.0f)));
            for (uint32_t s = 0; s < per_pixel; ++s)
                for (int pix = 0; pix < 256; ++pix) {
                    int px, py; film_tile_pixel(pix, x0, y0, px, py);
                    if (px >= W || py >= H) continue;
                    Rng rng; rng_seed(rng, (uint64_t) py * (uint64_t) W + (uint64_t) px, (uint64_t) s);      /* first_vertex */
                    const f2 j = rng_next_2d(rng);
                    one(tile, mk2((float) px + j.x, (float) py + j.y));
                }
        }
    });
    for (auto &t : th) t.join();
    for (int k = 0; k < 8; ++k) { out[k] = 0; for (unsigned t = 0; t < nt; ++t) out[k] += acc[t][k]; }
    return 0;
}

} // extern "C"
