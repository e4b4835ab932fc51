/*
 * lights.h -- delta lights (point, spot, directional), per-lane code (include/nori_hip.h, "Delta lights").
 *
 * Lights without geometry: n_lights records of 48 bytes in device memory (LightRec, rt_types.h; DevScene::lights).  They are
 * n_lights more lights in the emitter pick of sample_direct (rt_path.h, kDeltaLit), between the area emitters and the environment.
 * Everything is float32 without contraction, / and sqrt the exact ones (rt_types.h), in the order the header states --
 * tests/delta_lights_ref.py restates it and the device is held to that bit for bit.
 */
#pragma once
#include "rt_sampling.h"

namespace nrt {

/* What light l sends towards the point p: the unit direction from p to the light, the shadow ray's maxt, the radiance term R
   (intensity, times the cone's falloff for a spot) and the squared distance the sample divides by (1 for a directional light,
   which has no distance; dist is then infinite).  False: no sample -- p lies at the light, or outside a spot's cone. */
NORI_HD bool light_incident(const LightRec &l, const f3 p, f3 &dir, float &maxt, f3 &R, float &dist2, float &dist) {
    R = mk3(l.intensity[0], l.intensity[1], l.intensity[2]);
    const f3 axis = mk3(l.direction[0], l.direction[1], l.direction[2]);
    if (l.type == kLightDirectional) {
        dir = -axis;
        maxt = kInf; dist2 = 1.0f; dist = kInf;
        return true;
    }
    const f3 dvec = mk3(l.position[0], l.position[1], l.position[2]) - p;
    dist2 = dot(dvec, dvec);
    if (dist2 == 0.0f) return false;
    dist = exact_sqrt(dist2);
    dir = dvec / dist;
    maxt = dist - kEpsilon;
    if (l.type == kLightSpot) {
        const float c = dot(axis, -dir);
        if (c <= l.cos_outer) return false;
        if (!(c >= l.cos_inner)) {      /* the falloff band: smoothstep of where c lies in it (a hard edge has no band: no quotient) */
            const float t = exact_div(c - l.cos_outer, l.cos_inner - l.cos_outer);
            const float fall = (t * t) * (3.0f - (2.0f * t));
            R = R * fall;
        }
    }
    return true;
}

} // namespace nrt
