/*
 * medium.h -- the homogeneous participating medium, per-lane code (include/nori_hip.h, "Homogeneous participating medium").
 *
 * One medium per context; it fills all space and the camera is inside it.  A grey extinction sigma_t, a single-scattering albedo and
 * a Henyey-Greenstein phase function with asymmetry g (g > 0: forward, along the ray's direction of travel).  Everything is float32
 * without contraction, / and sqrt the exact ones (rt_types.h), log / exp / sincos the pinned ones (rt_math.h), in the order the header
 * states -- tests/medium_ref.py restates it and the device is held to that bit for bit.  The record (MediumRec, rt_types.h) lies in
 * DevScene by value and carries what is derived from g once: a = 1 - g g, b = 1 + g g, g2 = 2 g, c = 1 - g.
 */
#pragma once
#include "rt_sampling.h"

namespace nrt {

/* the record of (sigma_t, albedo, g): |g| < 1e-3 is stored as exactly 0 (isotropic; the inversion divides by 2 g) */
NORI_HD MediumRec medium_record(float sigma_t, const float albedo[3], float g) {
    MediumRec m;
    m.sigma_t = sigma_t;
    m.albedo[0] = albedo[0]; m.albedo[1] = albedo[1]; m.albedo[2] = albedo[2];
    if (fabsf(g) < 1e-3f) g = 0.0f;
    const float g2 = g * g;
    m.g = g; m.a = 1.0f - g2; m.b = 1.0f + g2; m.g2 = 2.0f * g; m.c = 1.0f - g;
    m.on = 1u;
    return m;
}

/* HG(c), c = the cosine between the ray's direction of travel and the scattered direction */
NORI_HD float hg_eval(const MediumRec &m, float c) {
    if (m.g == 0.0f) return kInvFourPi;
    const float k = m.b - m.g2 * c;
    return exact_div(kInvFourPi * m.a, k * exact_sqrt(k));
}

/* the scattered direction in the frame whose z is the direction of travel */
NORI_HD f3 hg_sample_local(const MediumRec &m, f2 xi) {
    if (m.g == 0.0f) return square_to_uniform_sphere(xi);
    const float sq = exact_div(m.a, m.c + m.g2 * xi.x);
    float c = exact_div(m.b - sq * sq, m.g2);
    c = fminf(fmaxf(c, -1.0f), 1.0f);
    const float r = exact_sqrt(fmaxf(0.0f, 1.0f - c * c));
    float sn, cs;
    det_sincosf(2.0f * kPi * xi.y, &sn, &cs);
    return mk3(r * cs, r * sn, c);
}

/* the world direction (not renormalised) and its density, re-evaluated from that direction: phase sampling and emitter sampling
   agree on the density of a direction */
NORI_HD f3 hg_sample(const MediumRec &m, f3 d, f2 xi, float &pdf) {
    const f3 wo = to_world(make_frame(d), hg_sample_local(m, xi));
    pdf = hg_eval(m, dot(d, wo));
    return wo;
}

/* the free-flight distance xi selects: -log(1 - xi) / sigma_t.  xi = 0 gives -0 / sigma_t, whose sign exact_div does not pin
   (rt_types.h); the addition makes it +0 on every machine and changes no other value */
NORI_HD float medium_distance(const MediumRec &m, float xi) { return exact_div(-det_logf(1.0f - xi), m.sigma_t) + 0.0f; }

/* Tr(dist) = exp(-(sigma_t dist)) */
NORI_HD float medium_tr(const MediumRec &m, float dist) { return det_expf(-(m.sigma_t * dist)); }

} // namespace nrt
