/*
 * wavefront_lights.hip -- wf_shade and wf_finish (wf_path_kernels.h) for contexts with delta lights (lights.h).
 *
 * Three general variants for each of path_ems and path_mis, on the full path record: MATSET = kAnyBsdf | kTextured | kDeltaLit
 * (rt_path.h) -- every BSDF, textured albedos, the lights --, that with kEnvLit for a context that also has an environment map, and
 * that with kMedium for one that also has a medium.  As in wavefront_env.hip and wavefront_medium.hip the kernels are instantiated
 * HERE and not in wavefront.hip, whose set of kernels stays the set it was; the text they are made of is wf_device.h's.
 * wavefront.hip's launch_shade / launch_finish call in, before the environment's and the medium's branches, for a scene whose
 * DevScene::n_lights is not zero and whose integrator is path_ems or path_mis (nori_hip_set_lights refuses every other).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "wf_device.h"

namespace {

constexpr int kLitSet = kAnyBsdf | kTextured | kDeltaLit;

template <int INTEG, int SET>
void shade_lit(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, int mode, int grid_, hipStream_t s) {
    const dim3 grid(grid_ * (kB / kSB)), block(kSB);
    const bool lds_tables = shade_tables_fit(sc);
#define SH(F) if (lds_tables) hipLaunchKernelGGL((wf_shade<INTEG, F, true, SET>), grid, block, 0, s, sc, b, cur, bt); \
              else hipLaunchKernelGGL((wf_shade<INTEG, F, false, SET>), grid, block, 0, s, sc, b, cur, bt)
    if (mode == kFreshOnly) { SH(kFreshOnly); } else if (mode == kMixed) { SH(kMixed); } else { SH(kStoredOnly); }
#undef SH
}

template <int INTEG>
void shade_lit_set(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, int mode, int grid, hipStream_t s) {
    if (sc.medium.on) shade_lit<INTEG, kLitSet | kMedium>(sc, b, cur, bt, mode, grid, s);
    else if (sc.env) shade_lit<INTEG, kLitSet | kEnvLit>(sc, b, cur, bt, mode, grid, s);
    else shade_lit<INTEG, kLitSet>(sc, b, cur, bt, mode, grid, s);
}

template <int INTEG>
void finish_lit_set(const DevScene &sc, const WfBuf &b, int cur, const WfBatch &bt, bool count, int grid_, hipStream_t s) {
    const dim3 grid(grid_), block(kB);
    const size_t lds = (size_t) LdsStackW<16, true>::kLdsEntries * kB * sizeof(int);
    if (sc.medium.on) hipLaunchKernelGGL((wf_finish<INTEG, kLitSet | kMedium>), grid, block, lds, s, sc, b, cur, bt, (int) count);
    else if (sc.env) hipLaunchKernelGGL((wf_finish<INTEG, kLitSet | kEnvLit>), grid, block, lds, s, sc, b, cur, bt, (int) count);
    else hipLaunchKernelGGL((wf_finish<INTEG, kLitSet>), grid, block, lds, s, sc, b, cur, bt, (int) count);
}

} // namespace

namespace nrt {

void wf_lights_launch_shade(const DevScene &sc, const void *wf_buf, int cur, const void *batch, int mode, int grid, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    switch (sc.integrator.type) {
    case INT_EMS: shade_lit_set<INT_EMS>(sc, b, cur, bt, mode, grid, s); break;
    case INT_MIS: shade_lit_set<INT_MIS>(sc, b, cur, bt, mode, grid, s); break;
    default: break;      /* (the caller asks for these two only) */
    }
}

void wf_lights_launch_finish(const DevScene &sc, const void *wf_buf, int cur, const void *batch, bool count, int grid, hipStream_t s) {
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    switch (sc.integrator.type) {
    case INT_EMS: finish_lit_set<INT_EMS>(sc, b, cur, bt, count, grid, s); break;
    case INT_MIS: finish_lit_set<INT_MIS>(sc, b, cur, bt, count, grid, s); break;
    default: break;
    }
}

} // namespace nrt
