/*
 * grid_medium.h -- the heterogeneous (voxel grid) participating medium, per-lane code (include/nori_hip.h, "Grid medium").
 *
 * One grid medium per context, as an alternative to the homogeneous one of medium.h: an axis-aligned box [bmin, bmax] of
 * nx ny nz voxels of float32 density rho, x fastest, PIECEWISE CONSTANT; the extinction of a voxel is sigma = sigma_scale rho and
 * outside the box there is vacuum.  The optical depth along a ray is then an exact finite sum over the voxels a 3-D DDA visits: the
 * free flight is sampled by analytic inversion (regular tracking) from the ONE number the homogeneous medium draws, and the
 * transmittance is exp(-tau) without a random number.  Albedo and phase function are medium.h's (DevScene::medium).
 *
 * Everything is float32 without contraction, the reciprocal and the quotient the exact ones (rt_types.h), log / exp the pinned ones
 * (rt_math.h), in the order the header states -- tests/grid_medium_ref.py restates it and the device is held to that bit for bit.
 * Minima, maxima and clamps are written as selects on ONE comparison, so that signed zeros take one way on every machine.
 */
#pragma once
#include "medium.h"

namespace nrt {

/* an axis with |d_a| below this (2^-40) is PARALLEL: it never steps, and its reciprocal is never taken */
constexpr float kGridParallel = 9.094947017729282e-13f;

struct GridWalk {
    float tau;          /* the optical depth accumulated: over the whole clipped ray, or up to the event's voxel */
    float s;            /* the event's distance (event), else +inf */
    int32_t steps;      /* voxels visited */
    bool event;
};

/* The walk of the ray (o, d) over [0, tmax]: clip to the box by slabs, then visit the voxels in order, tau += sigma_i max(0, t_end -
   t_cur).  It stops in the first voxel with sigma_i > 0 in which the sum reaches tau_stop (+inf: never) and gives
   s = (t_cur + (tau_stop - tau) / sigma_i) + 0 there.  Plane crossings are made from the INTEGER plane index each time -- nothing is
   accumulated along the ray --, ties step x, then y, then z, and the loop takes nx + ny + nz trips at the most: every trip but the
   last moves one index by one towards the face its axis leaves through.  The voxel index is clamped where it is made and tested
   before it moves, so rho is never read outside its nx ny nz entries whatever the ray. */
NORI_HD GridWalk grid_walk(const GridMediumRec &g, const f3 o, const f3 d, const float tmax, const float tau_stop) {
    GridWalk w;
    w.tau = 0.0f; w.s = kInf; w.steps = 0; w.event = false;
    const float oa[3] = {o.x, o.y, o.z}, da[3] = {d.x, d.y, d.z};
    float inv[3];
    int32_t step[3], i[3];
    float t0 = 0.0f, t1 = tmax;
    bool miss = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool par = fabsf(da[a]) < kGridParallel;
        inv[a] = exact_rcp(par ? 1.0f : da[a]);
        step[a] = par ? 0 : (da[a] > 0.0f ? 1 : -1);
        /* a parallel axis: inside its slab means bmin <= o < bmax -- a point on a plane belongs to the voxel ABOVE it */
        if (par && !(oa[a] >= g.bmin[a] && oa[a] < g.bmax[a])) miss = true;
        if (!par) {
            const float ta = (g.bmin[a] - oa[a]) * inv[a], tb = (g.bmax[a] - oa[a]) * inv[a];
            const float tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
            t0 = tn > t0 ? tn : t0;
            t1 = tf < t1 ? tf : t1;
        }
    }
    if (miss || (step[0] == 0 && step[1] == 0 && step[2] == 0) || !(t0 < t1)) return w;
    /* the voxel of the entry point o + d t0 (a parallel axis: of o): floor, clamped; a point on a plane belongs to the voxel above it,
       whichever way the ray goes -- going down, its first segment is empty and the first step leaves it */
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = step[a] == 0 ? oa[a] : oa[a] + da[a] * t0;
        float c = floorf((p - g.bmin[a]) * g.inv_cell[a]);
        const float hi = (float) (g.n[a] - 1);
        c = c >= 0.0f ? c : 0.0f;
        c = c <= hi ? c : hi;
        i[a] = (int32_t) c;
    }
    float t_cur = t0, tau = 0.0f;
    const int32_t cap = g.n[0] + g.n[1] + g.n[2];
    for (int32_t trip = 0; trip < cap; ++trip) {
        float t[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int32_t k = i[a] + (step[a] > 0 ? 1 : 0);
            const float plane = g.bmin[a] + (float) k * g.cell[a];
            t[a] = step[a] == 0 ? kInf : (plane - oa[a]) * inv[a];
        }
        const bool sx = t[0] <= t[1] && t[0] <= t[2];
        const bool sy = !sx && t[1] <= t[2];
        const float t_next = sx ? t[0] : (sy ? t[1] : t[2]);
        const float t_end = t_next < t1 ? t_next : t1;
        const float sigma = g.sigma_scale * g.rho[((size_t) i[2] * (size_t) g.n[1] + (size_t) i[1]) * (size_t) g.n[0] + (size_t) i[0]];
        const float len = t_end - t_cur;
        const float tau_new = tau + sigma * (len > 0.0f ? len : 0.0f);
        w.steps++;
        if (sigma > 0.0f && tau_new >= tau_stop) {
            w.event = true;
            w.s = (t_cur + exact_div(tau_stop - tau, sigma)) + 0.0f;
            break;
        }
        tau = tau_new;
        if (!(t_next < t1)) break;
        t_cur = t_next > t_cur ? t_next : t_cur;
        i[0] += sx ? step[0] : 0; i[1] += sy ? step[1] : 0; i[2] += (sx || sy) ? 0 : step[2];
        if (i[0] < 0 || i[0] >= g.n[0] || i[1] < 0 || i[1] >= g.n[1] || i[2] < 0 || i[2] >= g.n[2]) break;
    }
    w.tau = tau;
    return w;
}

/* the free flight xi selects on the ray (o, d) over [0, tmax]: true and s, or false -- no event before tmax or the box's far side */
NORI_HD bool grid_distance(const GridMediumRec &g, const f3 o, const f3 d, const float tmax, const float xi, float &s) {
    const GridWalk w = grid_walk(g, o, d, tmax, -det_logf(1.0f - xi));
    s = w.s;
    return w.event;
}

/* Tr over [0, dist] = exp(-tau); dist may be infinite, the box bounds the walk */
NORI_HD float grid_tr(const GridMediumRec &g, const f3 o, const f3 d, const float dist) {
    return det_expf(-grid_walk(g, o, d, dist, kInf).tau);
}

} // namespace nrt
