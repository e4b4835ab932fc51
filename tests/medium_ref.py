"""The homogeneous medium (include/nori_hip.h, "Homogeneous participating medium") restated in numpy: float32, every operation in
the order the header states it, no contraction.  / and sqrt of numpy's float32 are the correctly rounded ones; log, exp and sincos
are parameters -- by default the CPU restatement of the pinned functions (Oracle.libm), the GPU tests pass the device's own
(Renderer.arith), which tests/test_gpu_arith.py holds to the former bit for bit.

walk() restates Li as a whole for scenes of diffuse meshes without vertex normals and area emitters: the state machine of rt_path.h,
vectorised over the paths, every closest-hit and shadow answer asked of the renderer's own intersect()."""
from __future__ import annotations

import numpy as np

F = np.float32
KINVPI = F(0.31830988618379067154)
KINVFOURPI = F(0.07957747154594766788)
KPI = F(3.14159265358979323846)
KEPS = F(1e-4)
NO_HIT = 0xFFFFFFFF
MAX_VERTICES = 64
DRAWS_PER_VERTEX = 8      # distance 1, Russian roulette 1, emitter 4, BSDF / phase 2


def _libm(op):
    from tests.backends import Oracle
    return lambda x: Oracle.libm(op, np.ascontiguousarray(x, F))


def default_log(x):
    return _libm("log")(x)


def default_exp(x):
    return _libm("exp")(x)


def default_sincos(x):
    return _libm("sin")(x), _libm("cos")(x)


def device_functions(r):
    """(log, exp, sincos) of the device itself, for the GPU tests"""
    return (lambda x: r.arith("log", x)), (lambda x: r.arith("exp", x)), (lambda x: (r.arith("sin", x), r.arith("cos", x)))


def dot(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


class Medium:
    """sigma_t, albedo[3], g and what is derived from g once, in float32"""

    def __init__(self, sigma_t, albedo, g=0.0):
        self.sigma_t = F(sigma_t)
        self.albedo = np.asarray(albedo, F).reshape(3)
        g = F(g)
        if abs(g) < F(1e-3):
            g = F(0.0)
        g2 = g * g
        self.g, self.A, self.B, self.G2, self.C = g, F(1.0) - g2, F(1.0) + g2, F(2.0) * g, F(1.0) - g


def hg_eval(m: Medium, c):
    c = np.asarray(c, F)
    if m.g == 0:
        return np.full(c.shape, KINVFOURPI, F)
    k = m.B - m.G2 * c
    return ((KINVFOURPI * m.A) / (k * np.sqrt(k))).astype(F)


def coordinate_system(a):
    """(b, c) of src/common.cpp:248-257 for unit vectors a [n, 3]"""
    a = np.asarray(a, F)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    zero = np.zeros_like(x)
    one = F(1.0)
    with np.errstate(all="ignore"):      # (the branch not taken may divide by zero: an axis)
        inv1 = one / np.sqrt(x * x + z * z)
        inv2 = one / np.sqrt(y * y + z * z)
        c1 = np.stack([z * inv1, zero, -x * inv1], -1)
        c2 = np.stack([zero, z * inv2, -y * inv2], -1)
    c = np.where((np.abs(x) > np.abs(y))[:, None], c1, c2).astype(F)
    return cross(c, a).astype(F), c


def to_world(s, t, n, v):
    return ((s * v[:, 0:1] + t * v[:, 1:2]) + n * v[:, 2:3]).astype(F)


def uniform_sphere(xi, sincos):
    xi = np.asarray(xi, F)
    z = F(1.0) - F(2.0) * xi[:, 0]
    r = np.sqrt(np.maximum(F(0.0), F(1.0) - z * z))
    sn, cs = sincos((F(2.0) * KPI) * xi[:, 1])
    return np.stack([r * cs, r * sn, z], -1).astype(F)


def hg_sample(m: Medium, d, xi, sincos=default_sincos):
    """(wo [n, 3], pdf [n]) for directions of travel d [n, 3] and samples xi [n, 2]"""
    d, xi = np.asarray(d, F).reshape(-1, 3), np.asarray(xi, F).reshape(-1, 2)
    if m.g == 0:
        local = uniform_sphere(xi, sincos)
    else:
        sq = m.A / (m.C + m.G2 * xi[:, 0])
        c = (m.B - sq * sq) / m.G2
        c = np.minimum(np.maximum(c, F(-1.0)), F(1.0))
        r = np.sqrt(np.maximum(F(0.0), F(1.0) - c * c))
        sn, cs = sincos((F(2.0) * KPI) * xi[:, 1])
        local = np.stack([r * cs, r * sn, c], -1).astype(F)
    s, t = coordinate_system(d)
    wo = to_world(s, t, d, local)
    return wo, hg_eval(m, dot(d, wo))


def distance(m: Medium, xi, log=default_log):
    """s = (-log(1 - xi)) / sigma_t + 0: the addition turns the -0 of xi = 0 into +0 and changes nothing else"""
    xi = np.asarray(xi, F)
    return ((-log(F(1.0) - xi)) / m.sigma_t + F(0.0)).astype(F)


def transmittance(m: Medium, dist, exp=default_exp):
    return exp(-(m.sigma_t * np.asarray(dist, F))).astype(F)


# ------------------------------------------------------------------ Li, restated
def walk(r, scene, medium, integrator, rays, floats, log=default_log, exp=default_exp, sincos=default_sincos, max_vertices=MAX_VERTICES):
    """(L [n, 3] float32, n_closest, n_shadow): Li of `rays` (the structured rays of r.sample_rays) in `scene` -- diffuse meshes
    without vertex normals, area emitters -- filled with `medium`, under path_mats / path_ems / path_mis.  floats[k]: the numbers
    path k draws, in order, from its first vertex on.  r answers every closest-hit and shadow query (r.intersect) and warps the
    cosine hemisphere (r.warp); r.emitter_tables() gives the CDFs the pick walks.  Every path must end within max_vertices (a hard
    cap, asserted: Russian roulette lets a path survive a vertex with the probability of its largest albedo component at most, so
    a caller whose albedos are close to 1 sizes the cap from that -- and floats has DRAWS_PER_VERTEX numbers per vertex of it)."""
    from tests import light_cases
    assert integrator in ("path_mats", "path_ems", "path_mis")
    assert all(m.bsdf.type == "diffuse" and m.normals is None for m in scene.meshes)
    EMS, MIS = integrator != "path_mats", integrator == "path_mis"
    n = rays.shape[0]
    floats = np.ascontiguousarray(floats, F)
    assert floats.shape[0] == n and floats.shape[1] >= max_vertices * DRAWS_PER_VERTEX
    tables = r.emitter_tables() if EMS else None
    nE = sum(1 for m in scene.meshes if m.radiance is not None)
    albedo_of = np.array([m.bsdf.albedo for m in scene.meshes], F)
    rad_of = np.array([m.radiance if m.radiance is not None else (0, 0, 0) for m in scene.meshes], F)
    is_em = np.array([m.radiance is not None for m in scene.meshes])
    inv_area = r.emitter_tables()["inv_area"].astype(F)
    one, zero = F(1.0), F(0.0)

    o, d = rays["o"].astype(F).copy(), rays["d"].astype(F).copy()
    mint, maxt = rays["mint"].astype(F).copy(), rays["maxt"].astype(F).copy()
    T, L = np.ones((n, 3), F), np.zeros((n, 3), F)
    pdf_mat, discrete = np.zeros(n, F), np.ones(n, bool)      # prev_measure == 2 for the camera ray
    depth, cur = np.zeros(n, np.int64), np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    n_closest = n_shadow = 0

    def draw(idx):
        v = floats[idx, cur[idx]]
        cur[idx] += 1
        return v

    def query(idx, org, dirs, lo, hi, shadow):
        q = np.zeros(idx.shape[0], rays.dtype)
        q["o"], q["d"], q["mint"], q["maxt"] = org, dirs, lo, hi
        return r.intersect(q, shadow=shadow)

    def emitter_geometry(idx, at):
        """the emitter sample of paths idx seen from the points `at`: (ok, dir, dist, dist2, cosY, pdfA, rad), four draws"""
        xs = np.stack([draw(idx), draw(idx), draw(idx), draw(idx)], -1)
        if nE == 0:
            z = np.zeros(idx.shape[0], F)
            return np.zeros(idx.shape[0], bool), np.zeros((idx.shape[0], 3), F), z, z, z, z, np.zeros((idx.shape[0], 3), F)
        mesh, tri, p = light_cases.pick_reference(scene, tables, xs)
        nrm = np.zeros((idx.shape[0], 3), F)
        for mi in np.unique(mesh):
            sel = mesh == mi
            m = scene.meshes[int(mi)]
            v = m.positions[m.indices[tri[sel]].astype(np.int64)].astype(F)
            c = cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(F)
            nrm[sel] = c / np.sqrt(dot(c, c))[:, None]
        dvec = (p - at).astype(F)
        dist2 = dot(dvec, dvec)
        dist = np.sqrt(dist2)
        with np.errstate(all="ignore"):
            dirs = (dvec / dist[:, None]).astype(F)
        cosY = dot(nrm, -dirs)
        pdfA = inv_area[mesh] * (one / F(nE))
        return cosY > 0, dirs, dist, dist2, cosY, pdfA, rad_of[mesh]

    for _ in range(max_vertices):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        its = query(idx, o[idx], d[idx], mint[idx], maxt[idx], False)
        n_closest += idx.size
        found = its["mesh"] != NO_HIT
        di = d[idx]
        s = distance(medium, draw(idx), log)
        med = ~found | (s < its["t"])
        # what a vertex leaves behind for its paths (positions within idx)
        k = idx.size
        origin, cont = np.zeros((k, 3), F), np.zeros((k, 3), F)
        ends = np.zeros(k, bool)                   # the path ends at this vertex, before any shadow ray
        dead = np.zeros(k, bool)                   # no continuation (after the shadow ray, if any)
        shadow = np.zeros(k, bool)
        sh_dir, sh_maxt, Ld = np.zeros((k, 3), F), np.zeros(k, F), np.zeros((k, 3), F)
        Tn, pm = T[idx].copy(), pdf_mat[idx].copy()

        # ---------------- medium vertices
        a = np.nonzero(med)[0]
        if a.size:
            ga = idx[a]
            origin[a] = (o[ga] + di[a] * s[a][:, None]).astype(F)
            Tn[a] = Tn[a] * medium.albedo[None, :]
            black = (Tn[a] == 0).all(axis=1)
            ends[a[black]] = True
            go = a[~black]
            rr = go[depth[idx[go]] >= 3]
            if rr.size:
                q = np.minimum(Tn[rr].max(axis=1) * one * one, F(0.99))
                keep = draw(idx[rr]) < q
                Tn[rr] = (Tn[rr] / q[:, None]).astype(F)
                ends[rr[~keep]] = True
            go = go[~ends[go]]
            if EMS and go.size:
                ok, dirs, dist, dist2, cosY, pdfA, rad = emitter_geometry(idx[go], origin[go])
                with np.errstate(all="ignore"):
                    ph = hg_eval(medium, dot(di[go], dirs))
                    pdf_em = (pdfA * dist2) / cosY
                    ld = ((ph[:, None] * rad) * (cosY / (dist2 * pdfA))[:, None]) * transmittance(medium, dist, exp)[:, None]
                    w = np.where(pdf_em + ph > 0, pdf_em / (pdf_em + ph), zero).astype(F) if MIS else np.ones(go.size, F)
                    val = ((Tn[go] * ld) * w[:, None]).astype(F)
                g_ok = go[ok]
                shadow[g_ok] = True
                sh_dir[g_ok], sh_maxt[g_ok], Ld[g_ok] = dirs[ok], (dist - KEPS)[ok], val[ok]
            if go.size:
                xi = np.stack([draw(idx[go]), draw(idx[go])], -1)
                wo, pdf = hg_sample(medium, di[go], xi, sincos)
                cont[go] = wo
                pm[go] = pdf if MIS else zero
                discrete[idx[go]] = False
                depth[idx[go]] += 1

        # ---------------- surface vertices
        b = np.nonzero(~med)[0]
        if b.size:
            gb = idx[b]
            mesh = its["mesh"][b].astype(np.int64)
            fs, ft, fn = its["sh_s"][b].astype(F), its["sh_t"][b].astype(F), its["sh_n"][b].astype(F)
            origin[b] = its["p"][b]
            db = di[b]
            wi_z = dot(-db, fn)
            front = wi_z > 0
            em = is_em[mesh]
            # emission reached by BSDF / phase sampling
            wMat = np.ones(b.size, F)
            weighted = EMS & ~discrete[gb]
            if EMS:
                if not MIS:
                    wMat[weighted] = zero
                else:
                    tt = its["t"][b].astype(F)
                    with np.errstate(all="ignore"):
                        pdfA = inv_area[mesh] / F(max(nE, 1))
                        pdfEm = np.where(front, ((pdfA * tt) * tt) / wi_z, zero).astype(F)
                        wm = np.where(pm[b] + pdfEm > 0, pm[b] / (pm[b] + pdfEm), zero).astype(F)
                    sel = weighted & em
                    wMat[sel] = wm[sel]
            add = em & (wMat > 0)
            le = np.where(front[:, None], rad_of[mesh], zero).astype(F)
            Lb = L[gb]
            Lb[add] = (Lb[add] + (Tn[b][add] * le[add]) * wMat[add][:, None]).astype(F)
            L[gb] = Lb
            rr = b[depth[gb] >= 3]
            if rr.size:
                q = np.minimum(Tn[rr].max(axis=1) * one * one, F(0.99))
                keep = draw(idx[rr]) < q
                Tn[rr] = (Tn[rr] / q[:, None]).astype(F)
                ends[rr[~keep]] = True
            live = ~ends[b]
            go = b[live]
            if EMS and go.size:
                ok, dirs, dist, dist2, cosY, pdfA, rad = emitter_geometry(idx[go], origin[go])
                woz = dot(dirs, fn[live])
                ok = ok & front[live] & (woz > 0)                          # bsdf_eval of a diffuse surface
                alb = albedo_of[mesh[live]]
                ok = ok & ~(alb == 0).all(axis=1)                          # (an all-zero f is rejected)
                with np.errstate(all="ignore"):
                    pdf_em = (pdfA * dist2) / cosY
                    pdf_bsdf = KINVPI * woz
                    ld = (((alb * KINVPI) * rad) * ((woz * cosY) / (dist2 * pdfA))[:, None]) * transmittance(medium, dist, exp)[:, None]
                    w = np.where(pdf_em + pdf_bsdf > 0, pdf_em / (pdf_em + pdf_bsdf), zero).astype(F) if MIS else np.ones(go.size, F)
                    val = ((Tn[go] * ld) * w[:, None]).astype(F)
                g_ok = go[ok]
                shadow[g_ok] = True
                sh_dir[g_ok], sh_maxt[g_ok], Ld[g_ok] = dirs[ok], (dist - KEPS)[ok], val[ok]
            if go.size:
                xi = np.stack([draw(idx[go]), draw(idx[go])], -1)
                wo = r.warp("cosine_hemisphere", xi)
                alb = albedo_of[mesh[live]]
                dd = ~front[live] | (alb == 0).all(axis=1)                 # bsdf_sample returned zero: no continuation
                dead[go[dd]] = True
                g2 = go[~dd]
                Tn[g2] = Tn[g2] * alb[~dd]
                cont[g2] = to_world(fs[live][~dd], ft[live][~dd], fn[live][~dd], wo[~dd])
                pm[g2] = (KINVPI * wo[~dd][:, 2]) if MIS else zero
                discrete[idx[g2]] = False
                depth[idx[g2]] += 1

        # ---------------- the shadow rays, then what goes on
        sh = np.nonzero(shadow & ~ends)[0]
        if sh.size:
            ans = query(idx[sh], origin[sh], sh_dir[sh], np.full(sh.size, KEPS, F), sh_maxt[sh], True)
            n_shadow += sh.size
            lit = ans["mesh"] == NO_HIT
            g = idx[sh[lit]]
            L[g] = (L[g] + Ld[sh[lit]]).astype(F)
        T[idx], pdf_mat[idx] = Tn, pm
        stop = ends | dead
        alive[idx[stop]] = False
        go = ~stop
        o[idx[go]], d[idx[go]] = origin[go], cont[go]
        mint[idx[go]], maxt[idx[go]] = KEPS, F(np.inf)
    assert not alive.any(), f"{int(alive.sum())} paths still alive after {max_vertices} vertices"
    return L, n_closest, n_shadow
