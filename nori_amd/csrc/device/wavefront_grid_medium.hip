/*
 * wavefront_grid_medium.hip -- wf_shade and wf_finish (wf_path_kernels.h) for contexts with a grid medium (grid_medium.h).
 *
 * Two general sets on the full path record: MATSET = kAnyBsdf | kTextured | kMedium | kGridMedium (rt_path.h) -- every BSDF,
 * textured albedos, the medium's vertex code, the grid's walk -- for path_mats, path_ems and path_mis, and that with kDeltaLit for
 * path_ems and path_mis in a context that also has delta lights.  As in wavefront_medium.hip and wavefront_lights.hip the kernels
 * are instantiated HERE and not in wavefront.hip, whose set of kernels stays the set it was; the text they are made of is
 * wf_device.h's.  wavefront.hip's launch_shade / launch_finish call in, before the lights' and the homogeneous medium's branches,
 * for a scene whose DevScene::gmed.rho is not null and whose integrator is one of the three.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "wf_device.h"

namespace {

constexpr int kGridSet = kAnyBsdf | kTextured | kMedium | kGridMedium;

template <int INTEG, int SET>
void shade_grid(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, int mode, int grid_, hipStream_t s) {
    const dim3 grid(grid_ * (kB / kSB)), block(kSB);
    const bool lds_tables = shade_tables_fit(sc);
#define SH(F) if (lds_tables) hipLaunchKernelGGL((wf_shade<INTEG, F, true, SET>), grid, block, 0, s, sc, b, cur, bt); \
              else hipLaunchKernelGGL((wf_shade<INTEG, F, false, SET>), grid, block, 0, s, sc, b, cur, bt)
    if (mode == kFreshOnly) { SH(kFreshOnly); } else if (mode == kMixed) { SH(kMixed); } else { SH(kStoredOnly); }
#undef SH
}

template <int INTEG, int SET>
void finish_grid(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, bool count, int grid_, hipStream_t s) {
    const dim3 grid(grid_), block(kB);
    const size_t lds = (size_t) LdsStackW<16, true>::kLdsEntries * kB * sizeof(int);
    hipLaunchKernelGGL((wf_finish<INTEG, SET>), grid, block, lds, s, sc, b, cur, bt, (int) count);
}

} // namespace

namespace nrt {

void wf_grid_medium_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    const bool lit = sc.n_lights != 0u;      /* (nori_hip_set_lights refuses path_mats) */
    switch (sc.integrator.type) {
    case INT_MATS: shade_grid<INT_MATS, kGridSet>(sc, b, cur, bt, mode, grid, s); break;
    case INT_EMS: if (lit) shade_grid<INT_EMS, kGridSet | kDeltaLit>(sc, b, cur, bt, mode, grid, s); else shade_grid<INT_EMS, kGridSet>(sc, b, cur, bt, mode, grid, s); break;
    case INT_MIS: if (lit) shade_grid<INT_MIS, kGridSet | kDeltaLit>(sc, b, cur, bt, mode, grid, s); else shade_grid<INT_MIS, kGridSet>(sc, b, cur, bt, mode, grid, s); break;
    default: break;      /* (the caller asks for the path integrators only) */
    }
}

void wf_grid_medium_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    const bool lit = sc.n_lights != 0u;
    switch (sc.integrator.type) {
    case INT_MATS: finish_grid<INT_MATS, kGridSet>(sc, b, cur, bt, count, grid, s); break;
    case INT_EMS: if (lit) finish_grid<INT_EMS, kGridSet | kDeltaLit>(sc, b, cur, bt, count, grid, s); else finish_grid<INT_EMS, kGridSet>(sc, b, cur, bt, count, grid, s); break;
    case INT_MIS: if (lit) finish_grid<INT_MIS, kGridSet | kDeltaLit>(sc, b, cur, bt, count, grid, s); else finish_grid<INT_MIS, kGridSet>(sc, b, cur, bt, count, grid, s); break;
    default: break;
    }
}

} // namespace nrt
