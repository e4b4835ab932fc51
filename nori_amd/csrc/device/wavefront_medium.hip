/*
 * wavefront_medium.hip -- wf_shade and wf_finish (wf_path_kernels.h) for contexts with a homogeneous medium.
 *
 * One general variant per path integrator: MATSET = kAnyBsdf | kTextured | kMedium (rt_path.h) -- every BSDF, textured albedos, the
 * medium -- on the full path record.  As in wavefront_env.hip the kernels are instantiated HERE and not in wavefront.hip, whose set
 * of kernels stays the set it was; the text they are made of is wf_device.h's.  wavefront.hip's launch_shade / launch_finish call
 * in for a scene whose DevScene::medium is on and whose integrator is path_mats, path_ems or path_mis; everything else of a pass
 * -- wf_extend, the pool, the film -- is that unit's and does not know.  What the medium variant needs that no other does is the
 * ORIGIN of the ray a vertex consumes (a scattering event lies at o + d s): wf_shade loads it from the stored record, or takes
 * the camera's for a new path; wf_finish has it in registers.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "wf_device.h"

namespace {

constexpr int kMediumSet = kAnyBsdf | kTextured | kMedium;

template <int INTEG>
void shade_medium(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, int mode, int grid_, hipStream_t s) {
    const dim3 grid(grid_ * (kB / kSB)), block(kSB);
    const bool lds_tables = shade_tables_fit(sc);
#define SH(F) if (lds_tables) hipLaunchKernelGGL((wf_shade<INTEG, F, true, kMediumSet>), grid, block, 0, s, sc, b, cur, bt); \
              else hipLaunchKernelGGL((wf_shade<INTEG, F, false, kMediumSet>), grid, block, 0, s, sc, b, cur, bt)
    if (mode == kFreshOnly) { SH(kFreshOnly); } else if (mode == kMixed) { SH(kMixed); } else { SH(kStoredOnly); }
#undef SH
}

} // namespace

namespace nrt {

void wf_medium_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    switch (sc.integrator.type) {
    case INT_MATS: shade_medium<INT_MATS>(sc, b, cur, bt, mode, grid, s); break;
    case INT_EMS: shade_medium<INT_EMS>(sc, b, cur, bt, mode, grid, s); break;
    case INT_MIS: shade_medium<INT_MIS>(sc, b, cur, bt, mode, grid, s); break;
    default: break;      /* (the caller asks for the path integrators only) */
    }
}

void wf_medium_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid_, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    const dim3 grid(grid_), block(kB);
    const size_t lds = (size_t) LdsStackW<16, true>::kLdsEntries * kB * sizeof(int);
    switch (sc.integrator.type) {
    case INT_MATS: hipLaunchKernelGGL((wf_finish<INT_MATS, kMediumSet>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
    case INT_EMS: hipLaunchKernelGGL((wf_finish<INT_EMS, kMediumSet>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
    case INT_MIS: hipLaunchKernelGGL((wf_finish<INT_MIS, kMediumSet>), grid, block, lds, s, sc, b, cur, bt, (int) count); break;
    default: break;
    }
}

} // namespace nrt
