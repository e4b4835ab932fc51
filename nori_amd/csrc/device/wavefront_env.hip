/*
 * wavefront_env.hip -- wf_shade and wf_finish (wf_path_kernels.h) for scenes with an environment map.
 *
 * One general variant per path integrator: MATSET = kAnyBsdf | kTextured | kEnvLit (rt_path.h) -- every BSDF, textured albedos, the
 * environment -- on the full path record.  The kernels are instantiated HERE and not in wavefront.hip, whose set of kernels stays
 * the set it was (the guard on it: tests/test_lens_cpu.py); the text they are made of is wf_device.h's, which both units include.
 * wavefront.hip's launch_shade / launch_finish call in for a scene whose DevScene::env is set and whose integrator is path_mats,
 * path_ems or path_mis; everything else of a pass -- wf_extend, the pool, the film -- is that unit's and does not know.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "wf_device.h"

namespace {

constexpr int kEnvSet = kAnyBsdf | kTextured | kEnvLit;

template <int INTEG>
void shade_env(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, int mode, int grid_, hipStream_t s) {
    const dim3 grid(grid_ * (kB / kSB)), block(kSB);
    const bool lds_tables = shade_tables_fit(sc);
#define SH(F) if (lds_tables) hipLaunchKernelGGL((wf_shade<INTEG, F, true, kEnvSet>), grid, block, 0, s, sc, b, cur, bt); \
              else hipLaunchKernelGGL((wf_shade<INTEG, F, false, kEnvSet>), grid, block, 0, s, sc, b, cur, bt)
    if (mode == kFreshOnly) { SH(kFreshOnly); } else if (mode == kMixed) { SH(kMixed); } else { SH(kStoredOnly); }
#undef SH
}

} // namespace

namespace nrt {

void wf_env_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    switch (sc.integrator.type) {
    case INT_MATS: shade_env<INT_MATS>(sc, b, cur, bt, mode, grid, s); break;
    case INT_EMS: shade_env<INT_EMS>(sc, b, cur, bt, mode, grid, s); break;
    case INT_MIS: shade_env<INT_MIS>(sc, b, cur, bt, mode, grid, s); break;
    default: break;      /* (the caller asks for the path integrators only) */
    }
}

void wf_env_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid_, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    const dim3 grid(grid_), block(kB);
    const size_t lds = (size_t) LdsStackW<16, true>::kLdsEntries * kB * sizeof(int);
    switch (sc.integrator.type) {
    case INT_MATS: hipLaunchKernelGGL((wf_finish<INT_MATS, kEnvSet>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
    case INT_EMS: hipLaunchKernelGGL((wf_finish<INT_EMS, kEnvSet>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
    case INT_MIS: hipLaunchKernelGGL((wf_finish<INT_MIS, kEnvSet>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
    default: break;
    }
}

} // namespace nrt
