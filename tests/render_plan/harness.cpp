/* The host-side render arithmetic of nori_amd/csrc/device/render_plan.h as a program of its own (tests/test_render_plan_cpu.py builds
 * it with g++, plain and under the sanitizers): reads one case per line from the file named on the command line, prints one line of
 * results per case.
 *   geo W H tile_mod tile_rem border                    -> tiles_x tiles_y n_sel_tiles tile_w
 *   chunks n_sel_tiles spp_count target_wgs             -> n_chunks chunk_spp
 *   cut spp_count n_sel_tiles cap                       -> spp_per_launch
 *   budget call_samples opt_paths opt_samples reference per_path per_sample usable (-1: unknown)   -> max_paths max_samples
 *   ladder max_paths max_samples reference per_path per_sample   -> the pair after every rung, then "end" ("endless" after 200 rungs) */
#include <cstdio>
#include <cstring>

#include "../../nori_amd/csrc/device/render_plan.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: harness <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        char cmd[16];
        long long v[7] = {0, 0, 0, 0, 0, 0, 0};
        const int n = sscanf(line, "%15s %lld %lld %lld %lld %lld %lld %lld", cmd, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) - 1;
        if (n < 0) continue;
        if (!strcmp(cmd, "geo") && n == 5) {
            const render_plan::TileGeometry g = render_plan::tile_geometry((int) v[0], (int) v[1], (uint32_t) v[2], (uint32_t) v[3]);
            printf("%u %u %u %d\n", g.tiles_x, g.tiles_y, g.n_sel_tiles, render_plan::tile_width((int) v[4]));
        } else if (!strcmp(cmd, "chunks") && n == 3) {
            const render_plan::ChunkPlan p = render_plan::plan_chunks((uint32_t) v[0], (uint32_t) v[1], (uint32_t) v[2]);
            printf("%u %u\n", p.n_chunks, p.chunk_spp);
        } else if (!strcmp(cmd, "cut") && n == 3) {
            printf("%u\n", render_plan::spp_per_launch((uint32_t) v[0], (uint32_t) v[1], (size_t) v[2]));
        } else if (!strcmp(cmd, "budget") && n == 7) {
            const size_t usable = v[6] < 0 ? render_plan::kUsableUnknown : (size_t) v[6];
            const render_plan::WfBudget b = render_plan::wavefront_budget((size_t) v[0], (size_t) v[1], (size_t) v[2], v[3] != 0, (size_t) v[4], (size_t) v[5], usable);
            printf("%zu %zu\n", b.max_paths, b.max_samples);
        } else if (!strcmp(cmd, "ladder") && n == 5) {
            render_plan::WfBudget b;
            b.max_paths = (size_t) v[0]; b.max_samples = (size_t) v[1];
            int rungs = 0;
            while (rungs < 200 && render_plan::wavefront_oom_step(b, v[2] != 0, (size_t) v[3], (size_t) v[4])) { printf("%zu %zu ", b.max_paths, b.max_samples); ++rungs; }
            printf(rungs < 200 ? "end\n" : "endless\n");
        } else {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
    }
    fclose(f);
    return 0;
}
