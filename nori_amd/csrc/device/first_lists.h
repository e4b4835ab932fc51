/*
 * first_lists.h -- per-tile candidate lists for the camera rays of a pinhole camera (wavefront_first.hip), written as plain
 * per-lane code so that the kernel is a one-line wrapper and the CPU harness (tests/first_lists) runs the same steps as loops.
 *
 * The closest hit of a ray does not depend on the order in which triangles are tested (rt_trace.h, trav_leaf_step: on equal t the
 * larger global triangle id wins, whatever came first).  So a camera ray tested against any SUPERSET of the pair records its walk
 * could accept returns the walk's (t, u, v, tri), bit for bit.  The camera samples of a 16 x 16 tile share their origin O and a
 * narrow pyramid of directions; first_tile_walk collects, once per (tree, camera, tile), the leaf pairs whose boxes that pyramid
 * meets -- up to K of them; a tile that meets more is an OVERFLOW tile and its rays walk the tree as before.
 *
 * The pyramid.  camera_sample_ray (rt_trace.h) maps a sample position ps to the direction M normalize(S (ps.x inv_w, ps.y inv_h, 0))
 * with S = sample_to_camera (projective: lines go to lines) and M the upper 3 x 3 of camera_to_world.  Taking the float constants of
 * the CameraRec as exact reals, the directions of ps in the closed rectangle [x0, x0 + 16] x [y0, y0 + 16] (ps = (float) px + j with
 * j < 1 may round up to px + 1, hence closed) fill the convex cone over a planar quadrilateral: the intersection of four half
 * spaces N_k . (p - O) >= 0 whose planes pass through O and two neighbouring corner directions.  first_tile_frustum computes the
 * corner directions, the unit normals N_k and the depth functional G (G . (M d) = d.z: row 3 of the inverse of M) in binary64, whose
 * own rounding (2^-53) is nothing next to the margin below; O is computed exactly as camera_sample_ray computes it (same floats).
 *
 * The margin.  u = 2^-24.  What first_vertex / camera_sample_ray compute in binary32 differs from the exact direction as follows.
 *   1. r_i = ((m_i0 sx + m_i1 sy) + m_i2 0) + m_i3 with sx = fl(ps.x inv_w): every term passes at most four roundings (sx, the
 *      product, two sums; m_i2 0 and m_i3 1 are exact), so |dr_i| <= ((1 + u)^4 - 1) a_i <= 5 u a_i,  a_i = |m_i0| |sx| + |m_i1| |sy| + |m_i3|.
 *   2. nearP_i = fl(r_i / r_3), a correctly rounded quotient (rt_types.h, exact_div_by):
 *      |dnearP_i| <= (5 u a_i + |nearP_i| 5 u a_3) / (|r_3| - 5 u a_3) + u |nearP_i| =: e_i.
 *      a_i, |nearP_i| (a ratio of affine functions) and 1 / |r_3| each take their maximum over the rectangle at a corner (r_3 must
 *      keep its sign there, else no tile gets a list); |nearP| is at least the distance D of the quadrilateral's plane from the
 *      origin.  Angle between the computed and the exact nearP: theta_1 <= |e| / D.
 *   3. normalized(): the length is a common factor and turns nothing; the three quotients a_i / len are correctly rounded, each off
 *      by u |d_i|: theta_2 <= u.
 *   4. mat_vector: w_i = fl(m_i0 d.x + fl(m_i1 d.y + m_i2 d.z)), three roundings per term, |dw| <= 3 u |M|_F |d|; as an angle
 *      3 u |M|_F / sigma_min(M) <= 3 u kappa with kappa = |M|_F |M^-1|_F, which also bounds what M makes of theta_1 + theta_2.
 *   theta = 2 kappa (theta_1 + theta_2 + 3 u): the factor 2 pays for the second-order terms dropped above and for binary64.
 *   (A rigid camera_to_world has kappa = 3; the pa4 Cornell box at 1024^2 comes to theta ~ 4e-6 rad against a tile 8e-3 rad wide.)
 * A point P = O + t w of a computed ray w lies no further than theta |P - O| outside each exact plane.  The Moeller-Trumbore test
 * accepts such a ray only where it passes the triangle's PADDED box -- the premise every node test of the tree rests on
 * (rt_types.h, tri_box_pad: the pad covers the test's own rounding, grows with 1 / sin for slivers, and numerically collinear
 * triangles get unbounded boxes, which no plane test here culls); the walk's node test spends a tenth of that pad on its own
 * error (rt_trace.h, trav_inner_step), this one nothing, and still adds the pad of a well-shaped triangle once more:
 * pad_abs = kBoxPadRel x the diagonal of the root's box.  A box (centre c, half extent h) is culled by plane k iff
 *      N_k . (c - O) + sum_i |N_k,i| h_i  <  -(theta (|c - O|_1 + |h|_1) + pad_abs)
 * i.e. its farthest corner on the inner side is further out than any accepted point of the box can be (a point of the box is no
 * further from O than |c - O| + |h|, and the 1-norms, which cost no square root, are no less than the lengths).  A box that holds O
 * is never culled (the left side is >= 0), nor is one the pyramid merely touches.
 * Near / far: a hit has t in [fl(near invZ), fl(far invZ)], invZ = fl(1 / d.z), so t d.z lies in [near (1 - 3 u), far (1 + 3 u)];
 * its depth G . (P - O) = t (d.z + G . dw) with |G . dw| <= 3 u kappa, and d.z >= dz_min (the smallest corner value: |nearP| is
 * convex, its maximum is at a corner).  With eps_z = theta / dz_min + 8 u a box is culled iff its largest depth is below
 * near (1 - eps_z) - |G| pad_abs or its smallest above far (1 + eps_z) + |G| pad_abs.
 * margin_scale multiplies theta, eps_z and pad_abs: 1 in the product; the harness also runs the exactly representable axis-aligned
 * case at 0, so that the margin cannot hide a sign error.
 */
#pragma once
#include "rt_types.h"
#include "rt_trace.h"

namespace nrt {

constexpr uint32_t kFirstListOverflow = 0xffffffffu;      /* tile_count of a tile without a list */
constexpr int kFirstListStack = 64;                       /* deferred subtrees of first_tile_walk (trees are at most 64 deep) */
constexpr uint32_t kFirstListMaxK = 64u;                  /* the most pairs a list may be asked to hold */
constexpr uint32_t kFirstListDefaultK = 32u;              /* K of the product (the histogram and the sweep it was read from) */

struct FirstCamera {      /* what the tiles of one camera share */
    double O[3];          /* the rays' origin, as camera_sample_ray computes it */
    double M[9], G[3];    /* upper 3 x 3 of camera_to_world; row 3 of its inverse */
    double kappa, gnorm;
    double pad_abs;       /* kBoxPadRel x diagonal of the root's box */
    int ok;               /* 0: no tile gets a list (a degenerate camera, a tree without an inner root) */
};

struct FirstFrustum {     /* one tile */
    double N[4][3];       /* unit normals of the side planes, pointing inwards */
    double theta, eps_z;
    int ok;
};

NORI_HD double first_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
NORI_HD void first_cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

/* the (finite) union of the root's child boxes: its diagonal */
NORI_HD double first_root_diagonal(const DevScene &sc) {
    if (sc.root < 0 || sc.n_triangles == 0u) return 0.0;
    const f4 *nq = sc.nodes + (size_t) sc.root * kNodeQuads;
    const f4 q0 = nq[0], q1 = nq[1], q2 = nq[2];
    const double c[2][3] = {{q0.x, q0.y, q1.x}, {q0.z, q0.w, q1.y}}, h[2][3] = {{q2.x, q2.y, q1.z}, {q2.z, q2.w, q1.w}};
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    bool any = false;
    for (int k = 0; k < 2; ++k) {
        /* unbounded: box_centre_half (rt_types.h) stores such an axis as h = kBoxHalfInf -- 2^59, a finite number: a test against
           1e37 here took the subtree of the collinear triangles for a box 1e18 wide, and the pad that came of it culled nothing */
        const double inf = (double) kBoxHalfInf;
        if (!(h[k][0] < inf && h[k][1] < inf && h[k][2] < inf)) continue;
        any = true;
        for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], c[k][a] - h[k][a]); hi[a] = fmax(hi[a], c[k][a] + h[k][a]); }
    }
    if (!any) return 0.0;
    const double d[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    return sqrt(first_dot3(d, d));
}

NORI_HD void first_camera(const DevScene &sc, FirstCamera &C) {
    const CameraRec &cam = sc.camera;
    const f3 o = mat_point(cam.camera_to_world, mk3(0.0f, 0.0f, 0.0f));
    C.O[0] = o.x; C.O[1] = o.y; C.O[2] = o.z;
    const float *m = cam.camera_to_world;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C.M[3 * i + j] = m[4 * i + j];
    const double cx[3] = {C.M[0], C.M[3], C.M[6]}, cy[3] = {C.M[1], C.M[4], C.M[7]}, cz[3] = {C.M[2], C.M[5], C.M[8]};
    double yz[3], zx[3], xy[3];
    first_cross3(cy, cz, yz); first_cross3(cz, cx, zx); first_cross3(cx, cy, xy);
    const double det = first_dot3(cx, yz);
    double fro = 0.0, inv_fro = 0.0;
    for (int k = 0; k < 9; ++k) fro += C.M[k] * C.M[k];
    C.ok = (fabs(det) > 1e-300 && fro < 1e300 && sc.root >= 0 && sc.n_triangles != 0u && !sc.wide && !(cam.lens_radius > 0.0f)) ? 1 : 0;
    const double idet = C.ok ? 1.0 / det : 0.0;
    for (int a = 0; a < 3; ++a) { C.G[a] = xy[a] * idet; inv_fro += (yz[a] * yz[a] + zx[a] * zx[a] + xy[a] * xy[a]) * idet * idet; }
    C.kappa = sqrt(fro) * sqrt(inv_fro);
    C.gnorm = sqrt(first_dot3(C.G, C.G));
    C.pad_abs = (double) kBoxPadRel * first_root_diagonal(sc);
    if (!(C.kappa < 1e6) || !(fabs(o.x) < 1e37f) || !(fabs(o.y) < 1e37f) || !(fabs(o.z) < 1e37f)) C.ok = 0;
}

/* the pyramid of the tile whose first pixel is (x0, y0) */
NORI_HD void first_tile_frustum(const CameraRec &cam, const FirstCamera &C, int x0, int y0, double margin_scale, FirstFrustum &F) {
    const double u = 5.9604644775390625e-8;      /* 2^-24 */
    const float *S = cam.sample_to_camera;
    F.ok = 0; F.theta = 0.0; F.eps_z = 0.0;
    for (int k = 0; k < 4; ++k) for (int a = 0; a < 3; ++a) F.N[k][a] = 0.0;
    if (!C.ok) return;
    /* corners in the order (0,0), (1,0), (1,1), (0,1); index 4: the tile's centre */
    const double px[5] = {(double) x0, (double) (x0 + kTile), (double) (x0 + kTile), (double) x0, (double) x0 + 0.5 * kTile};
    const double py[5] = {(double) y0, (double) y0, (double) (y0 + kTile), (double) (y0 + kTile), (double) y0 + 0.5 * kTile};
    double P[5][3], D[5][3], amax[4] = {0, 0, 0, 0}, nmax[3] = {0, 0, 0}, wmin = 1e300, dzmin = 1e300;
    int wsign = 0;
    for (int k = 0; k < 5; ++k) {
        const double sx = px[k] * (double) cam.inv_w, sy = py[k] * (double) cam.inv_h;
        double r[4];
        for (int i = 0; i < 4; ++i) {
            r[i] = (double) S[4 * i] * sx + (double) S[4 * i + 1] * sy + (double) S[4 * i + 3];
            amax[i] = fmax(amax[i], fabs((double) S[4 * i]) * fabs(sx) + fabs((double) S[4 * i + 1]) * fabs(sy) + fabs((double) S[4 * i + 3]));
        }
        const int sg = r[3] > 0.0 ? 1 : (r[3] < 0.0 ? -1 : 0);
        if (sg == 0 || (wsign != 0 && sg != wsign)) return;
        wsign = sg;
        wmin = fmin(wmin, fabs(r[3]));
        for (int a = 0; a < 3; ++a) { P[k][a] = r[a] / r[3]; nmax[a] = fmax(nmax[a], fabs(P[k][a])); }
        const double len = sqrt(first_dot3(P[k], P[k]));
        if (!(len > 0.0)) return;
        const double d[3] = {P[k][0] / len, P[k][1] / len, P[k][2] / len};
        dzmin = fmin(dzmin, d[2]);
        for (int a = 0; a < 3; ++a) D[k][a] = C.M[3 * a] * d[0] + C.M[3 * a + 1] * d[1] + C.M[3 * a + 2] * d[2];
    }
    if (!(dzmin > 1e-3) || !(wmin > 5.0 * u * amax[3] * 2.0)) return;
    /* distance of the quadrilateral's plane from the origin */
    double e1[3], e2[3], pn[3];
    for (int a = 0; a < 3; ++a) { e1[a] = P[1][a] - P[0][a]; e2[a] = P[3][a] - P[0][a]; }
    first_cross3(e1, e2, pn);
    const double pnl = sqrt(first_dot3(pn, pn));
    if (!(pnl > 0.0)) return;
    const double dist = fabs(first_dot3(pn, P[0])) / pnl;
    if (!(dist > 0.0)) return;
    double e2sum = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double e = (5.0 * u * amax[a] + nmax[a] * 5.0 * u * amax[3]) / (wmin - 5.0 * u * amax[3]) + u * nmax[a];
        e2sum += e * e;
    }
    const double theta1 = sqrt(e2sum) / dist;
    F.theta = margin_scale * 2.0 * C.kappa * (theta1 + u + 3.0 * u);
    F.eps_z = margin_scale * (2.0 * C.kappa * (theta1 + u + 3.0 * u) / dzmin + 8.0 * u);
    if (!(F.theta < 1e-2)) return;      /* (a camera this ill-conditioned gets no lists) */
    for (int k = 0; k < 4; ++k) {
        double n[3];
        first_cross3(D[k], D[(k + 1) & 3], n);
        const double l = sqrt(first_dot3(n, n));
        if (!(l > 0.0)) return;
        const double s = first_dot3(n, D[4]) < 0.0 ? -1.0 / l : 1.0 / l;
        for (int a = 0; a < 3; ++a) F.N[k][a] = n[a] * s;
        if (!(first_dot3(F.N[k], D[4]) > 0.0)) return;
    }
    F.ok = 1;
}

/* may a ray of the tile meet the box (centre c, half extent h)? */
NORI_HD bool first_box_kept(const CameraRec &cam, const FirstCamera &C, const FirstFrustum &F, double margin_scale, const double c[3], const double h[3]) {
    const double v[3] = {c[0] - C.O[0], c[1] - C.O[1], c[2] - C.O[2]};
    const double pad = margin_scale * C.pad_abs;
    const double reach = F.theta * ((fabs(v[0]) + fabs(v[1]) + fabs(v[2])) + (h[0] + h[1] + h[2])) + pad;      /* 1-norms: no less than the lengths */
    for (int k = 0; k < 4; ++k) {
        const double s = first_dot3(F.N[k], v) + (fabs(F.N[k][0]) * h[0] + fabs(F.N[k][1]) * h[1] + fabs(F.N[k][2]) * h[2]);
        if (s < -reach) return false;
    }
    const double zc = first_dot3(C.G, v), zh = fabs(C.G[0]) * h[0] + fabs(C.G[1]) * h[1] + fabs(C.G[2]) * h[2];
    if (zc + zh < (double) cam.near_clip * (1.0 - F.eps_z) - C.gnorm * pad) return false;
    if (zc - zh > (double) cam.far_clip * (1.0 + F.eps_z) + C.gnorm * pad) return false;
    return true;
}

/* The tile's list: the pair records of every leaf the pyramid may meet, at most K of them, into out[0 .. K).  Returns their number,
   or kFirstListOverflow (more than K, no pyramid, or more deferred subtrees than the stack holds). */
NORI_HD uint32_t first_tile_walk(const DevScene &sc, const FirstCamera &C, const FirstFrustum &F, double margin_scale, uint32_t K, uint32_t *out) {
    if (!C.ok || !F.ok || K == 0u) return kFirstListOverflow;      /* (K = 0: no tile has a list, not even one that sees nothing) */
    int stack[kFirstListStack];
    int sp = 0;
    uint32_t n = 0;
    int link = sc.root;
    while (true) {
        if (link < 0) {      /* a leaf: ~link = (first_pair << 3) | (n_pairs - 1) */
            const uint32_t cursor = ~(uint32_t) link, first = cursor >> 3, cnt = (cursor & 7u) + 1u;
            if (n + cnt > K) return kFirstListOverflow;
            for (uint32_t k = 0; k < cnt; ++k) out[n + k] = first + k;
            n += cnt;
        } else {
            const f4 *nq = sc.nodes + (size_t) link * kNodeQuads;
            const f4 q0 = nq[0], q1 = nq[1], q2 = nq[2], q3 = nq[3];
            const double lc[3] = {q0.x, q0.y, q1.x}, rc[3] = {q0.z, q0.w, q1.y}, lh[3] = {q2.x, q2.y, q1.z}, rh[3] = {q2.z, q2.w, q1.w};
            const bool kl = first_box_kept(sc.camera, C, F, margin_scale, lc, lh), kr = first_box_kept(sc.camera, C, F, margin_scale, rc, rh);
            const int cl = (int) f2u(q3.x), cr = (int) f2u(q3.y);
            if (kl && kr) {
                if (sp >= kFirstListStack) return kFirstListOverflow;
                stack[sp++] = cr; link = cl; continue;
            }
            if (kl) { link = cl; continue; }
            if (kr) { link = cr; continue; }
        }
        if (sp == 0) break;
        link = stack[--sp];
    }
    return n;
}

/* One pair record against a camera ray: the update of trav_leaf_step<COUNT, false> for a closest-hit query -- same test, same tie
   rule (on equal t the larger global triangle id wins), written as the same selects. */
NORI_HD void first_pair_step(const f4 &q0, const f4 &q1, const f4 &q2, const f4 &q3, const f4 &q4, f3 o, f3 d, float mint, Hit &hit) {
    TriPairHit r;
    tri_pair_test(q0, q1, q2, q3, q4, o, d, mint, hit.t, r);
    const uint32_t gid0 = f2u(q4.z), gid1 = f2u(q4.w);
    const bool take0 = r.ok[0] && r.t[0] <= hit.t && !(r.t[0] == hit.t && hit.tri != kNoHit && gid0 < hit.tri);
    const float t0 = take0 ? r.t[0] : hit.t, u0 = take0 ? r.u[0] : hit.u, v0 = take0 ? r.v[0] : hit.v;
    const uint32_t tri0 = take0 ? gid0 : hit.tri;
    const bool take1 = r.ok[1] && r.t[1] <= t0 && !(r.t[1] == t0 && tri0 != kNoHit && gid1 < tri0);
    hit.t = take1 ? r.t[1] : t0; hit.u = take1 ? r.u[1] : u0; hit.v = take1 ? r.v[1] : v0; hit.tri = take1 ? gid1 : tri0;
}

/* a camera ray against a tile's list: what Accel::rayIntersect returns for it */
NORI_HD void first_list_trace(const DevScene &sc, const RayIn &ray, const uint32_t *pairs, uint32_t n, Hit &hit) {
    hit.tri = kNoHit; hit.mesh = kNoHit; hit.t = ray.maxt; hit.u = 0.0f; hit.v = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        const f4 *tq = sc.tris + (size_t) pairs[k] * kPairQuads;
        first_pair_step(tq[0], tq[1], tq[2], tq[3], tq[4], ray.o, ray.d, ray.mint, hit);
    }
}

} // namespace nrt
