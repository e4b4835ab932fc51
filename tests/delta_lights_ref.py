"""Delta lights (include/nori_hip.h, "Delta lights") restated in numpy: float32, every operation in the order the header states it,
no contraction; / and sqrt of numpy's float32 are the correctly rounded ones.

incident() is the twin's operation.  walk() restates Li of path_ems / path_mis for a scene with delta lights -- alone, with an
environment or with a medium -- for every material: the state machine of rt_path.h with kDeltaLit.  Nothing here comes from the
device under test: closest-hit and shadow answers and the BSDFs are the CPU oracle's, as tests/path_ref.py takes them, and its
pieces are path_ref's, medium_ref's, envmap_ref's, texture_ref's and light_cases.pick_reference by import.

walk() counts the events the new branches are taken at (EVENTS), and `mutate` names ONE deliberate departure from the
specification (MUTATIONS): tests/test_delta_lights_cpu.py shows that each changes the radiance of paths the GPU tests render."""
from __future__ import annotations

import numpy as np

from tests import medium_ref as mr, path_ref as pr
from tests.medium_ref import F, KEPS, KINVPI, NO_HIT, cross, dot, to_world
from tests.path_ref import _is_zero, _mis, _normalized, _to_local

POINT, SPOT, DIRECTIONAL = 0, 1, 2
TYPES = ("point", "spot", "directional")
DRAWS_PER_VERTEX = pr.DRAWS_PER_VERTEX

EVENTS = (
    "pick_point", "pick_spot", "pick_directional",      # a delta light picked, per type
    "emitter_hit_lights_count",                          # emitter hits whose MIS density carries lights in its count
    "env_pick_shifted",                                  # the environment picked at index n_emitters + n_lights
    "delta_at_medium_vertex",                            # a delta sample at a medium vertex
    "spot_in_band",                                      # a spot sample inside the falloff band
    "delta_sample_mis",                                  # a delta sample that asks for a shadow ray under path_mis
    "delta_shadow",                                      # a delta sample's shadow ray (point / spot: it has a distance)
    "delta_tr",                                          # a delta sample in a medium: Tr enters
)
# what the drawn lights of tests/path_fuzz.py's lit rounds are there to reach (the hand-made cases of tests/delta_light_cases.py are
# not asked for them): counted like EVENTS, never part of the contract of delta_light_cases.applicable
FUZZ_EVENTS = (
    "delta_outside_cone",                                # a delta pick without a sample: the point lies outside a spot's cone
    "delta_bsdf_zero",                                   # a delta pick rejected because the BSDF is zero (the light behind the surface)
    "delta_black_shadow",                                # a delta sample whose radiance is zero in every channel: its shadow ray is traced
    "delta_occluded",                                    # a delta sample whose shadow ray is occluded
    "hard_edge_lit",                                     # a sample of a spot with cos_inner == cos_outer
    "delta_medium_lens",                                 # a delta sample at a medium vertex of a path that began on a lens
)
# counted as well, asked of no drawn round (a vertex within 2e-4 of a light is not drawn; tests/test_gpu_delta_lights.py aims rays at one)
RARE_EVENTS = ("delta_empty_interval",)                  # a delta sample nearer than 2 kEpsilon: maxt < mint, traced, never occluded
MUTATIONS = {      # name -> the counter that is non-zero on every path the departure can change
    "emitter_hit_pdf_without_lights_in_count": "emitter_hit_lights_count",
    "env_at_unshifted_index": ("env_pick_shifted", "pick_point", "pick_spot", "pick_directional"),      # (the pick that index n_emitters was)
    "mis_weight_from_quotient": "delta_sample_mis",
    "no_falloff": "spot_in_band",
    "no_tr_on_delta": "delta_tr",
    "maxt_is_dist": "delta_shadow",
}


class Lights:
    """the lights as the context stores them: float32 arrays, the directions normalised (normalized() of rt_types.h), the fields a
    type does not use zero"""

    def __init__(self, lights):
        n = len(lights)
        self.n = n
        self.type = np.array([TYPES.index(l.type) for l in lights], np.int64)
        self.position = np.array([l.position for l in lights], F).reshape(n, 3)
        self.direction = _normalized(np.array([l.direction for l in lights], F).reshape(n, 3))
        self.intensity = np.array([l.intensity for l in lights], F).reshape(n, 3)
        self.cos_inner = np.array([l.cos_inner for l in lights], F)
        self.cos_outer = np.array([l.cos_outer for l in lights], F)
        self.position[self.type == DIRECTIONAL] = 0
        self.direction[self.type == POINT] = 0
        self.cos_inner[self.type != SPOT] = 0
        self.cos_outer[self.type != SPOT] = 0


def as_lights(lights):
    return lights if isinstance(lights, Lights) else Lights(list(lights))


def incident_full(lights, index, p, mutate=None):
    """(ok, dir, maxt, R, dist2, dist, band) of the lights `index` [n] seen from the points p [n, 3]; band: a spot sample inside
    the falloff band.  Rows that are not ok hold unspecified values."""
    L = as_lights(lights)
    index = np.asarray(index, np.int64)
    p = np.asarray(p, F).reshape(-1, 3)
    n = p.shape[0]
    t = L.type[index]
    one = F(1.0)
    R = L.intensity[index].copy()
    axis = L.direction[index]
    with np.errstate(all="ignore"):
        dvec = (L.position[index] - p).astype(F)
        dist2 = dot(dvec, dvec)
        dist = np.sqrt(dist2)
        dirs = (dvec / dist[:, None]).astype(F)
        maxt = (dist if mutate == "maxt_is_dist" else dist - KEPS).astype(F)
        ok = dist2 != 0
        c = dot(axis, -dirs)
        co, ci = L.cos_outer[index], L.cos_inner[index]
        spot = t == SPOT
        ok = ok & ~(spot & (c <= co))
        band = spot & ok & ~(c >= ci)
        tt = (c - co) / (ci - co)
        fall = (tt * tt) * (F(3.0) - (F(2.0) * tt))
    if mutate != "no_falloff":
        R[band] = (R[band] * fall[band][:, None]).astype(F)
    sun = t == DIRECTIONAL
    dirs[sun] = -axis[sun]
    maxt[sun] = F(np.inf)
    dist2[sun] = one
    dist[sun] = F(np.inf)
    ok[sun] = True
    assert dirs.dtype == F and R.dtype == F and maxt.dtype == F and dist2.dtype == F
    return ok, dirs, maxt, R, dist2, dist, band


def incident(lights, index, p):
    """the twin: (dir [n, 3], maxt [n], radiance [n, 3]), zeros where there is no sample"""
    ok, dirs, maxt, R, _, _, _ = incident_full(lights, index, p)
    z = ~ok
    dirs, maxt, R = dirs.copy(), maxt.copy(), R.copy()
    dirs[z], maxt[z], R[z] = 0, 0, 0
    return dirs, maxt, R


def walk(backend, scene, integrator, rays, floats, lights=None, medium=None, env=None, max_vertices=pr.MAX_VERTICES, mutate=None):
    """(L [n, 3] float32, n_closest, n_shadow, events): path_ref.walk's contract for path_ems / path_mis in a scene with the delta
    lights `lights` (a list of scene.Light; default scene.lights), filled with `medium` or lit by `env` (never both)."""
    from tests import light_cases, texture_ref
    from tests.backends import Oracle
    assert integrator in ("path_ems", "path_mis")
    assert mutate is None or mutate in MUTATIONS, mutate
    LT = as_lights(scene.lights if lights is None else lights)
    nD = LT.n
    assert nD > 0
    medium, env = pr.as_medium(medium), pr.as_env(env)
    assert medium is None or env is None
    MIS = integrator == "path_mis"
    MEDIUM, ENV = medium is not None, env is not None
    assert not (MEDIUM and (LT.type == DIRECTIONAL).any())
    n = rays.shape[0]
    floats = np.ascontiguousarray(floats, F)
    assert floats.shape[0] == n and floats.shape[1] >= max_vertices * DRAWS_PER_VERTEX
    one, zero = F(1.0), F(0.0)

    meshes = scene.meshes
    tables = pr.emitter_tables(scene)
    nE = sum(1 for m in meshes if m.radiance is not None)
    assert tables["n_emitters"] == nE
    nL = nE + nD + (1 if ENV else 0)              # the lights: area emitters, delta lights, the environment
    env_index = nE if mutate == "env_at_unshifted_index" else nE + nD
    pick_tables = dict(tables, n_emitters=nL, emitters=np.concatenate([tables["emitters"], np.zeros(nL - nE, np.uint32)]))
    inv_area = tables["inv_area"].astype(F)
    btype = np.array([{"diffuse": 0, "mirror": 1, "dielectric": 2, "microfacet": 3}[m.bsdf.type] for m in meshes])
    textured = np.array([m.albedo_texture is not None for m in meshes])
    assert not (textured & (btype != 0)).any()
    albedo_of = np.array([m.bsdf.albedo for m in meshes], F)
    rad_of = np.array([m.radiance if m.radiance is not None else (0, 0, 0) for m in meshes], F)
    is_em = np.array([m.radiance is not None for m in meshes])

    o, d = rays["o"].astype(F).copy(), rays["d"].astype(F).copy()
    mint, maxt = rays["mint"].astype(F).copy(), rays["maxt"].astype(F).copy()
    T, L = np.ones((n, 3), F), np.zeros((n, 3), F)
    eta, pdf_mat = np.ones(n, F), np.zeros(n, F)
    prev = np.full(n, 2, np.int64)                 # prev_measure: 2 for the camera ray
    depth, cur = np.zeros(n, np.int64), np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    n_closest = n_shadow = 0
    events = {k: np.zeros(n, np.int64) for k in EVENTS + FUZZ_EVENTS + RARE_EVENTS + ("vertices",)}
    LENS = scene.camera.aperture_radius > 0
    hard = (LT.type == SPOT) & (LT.cos_inner == LT.cos_outer)
    from_delta = np.zeros(n, bool)                 # the path's last emitter sample came from a delta light (and asks for a shadow ray)

    def draw(idx):
        v = floats[idx, cur[idx]]
        cur[idx] += 1
        return v

    def query(idx, org, dirs, lo, hi, shadow):
        q = np.zeros(idx.shape[0], rays.dtype)
        q["o"], q["d"], q["mint"], q["maxt"] = org, dirs, lo, hi
        return backend.intersect(q, shadow=shadow)

    def roulette(idx, Tn):
        e = eta[idx]
        m3 = np.maximum(Tn[:, 0], np.maximum(Tn[:, 1], Tn[:, 2]))
        p = np.minimum((m3 * e) * e, F(0.99))
        keep = draw(idx) < p
        with np.errstate(all="ignore"):
            return keep, (Tn / p[:, None]).astype(F)

    def surface_bsdf(mesh, alb, wi, wo):
        f, pdf = np.zeros((mesh.shape[0], 3), F), np.zeros(mesh.shape[0], F)
        for mi in np.unique(mesh):
            sel = mesh == mi
            b = meshes[int(mi)].bsdf
            if textured[mi]:
                up = (wi[sel, 2] > 0) & (wo[sel, 2] > 0)
                f[sel] = np.where(up[:, None], alb[sel] * KINVPI, zero)
                pdf[sel] = np.where(up, KINVPI * wo[sel, 2], zero)
            else:
                f[sel], pdf[sel] = Oracle.bsdf_eval(b, wi[sel], wo[sel]), Oracle.bsdf_pdf(b, wi[sel], wo[sel])
        return f, pdf

    def sample_direct(idx, at, med, di=None, frame=None, wi=None, mesh=None, alb=None):
        """sample_direct of rt_path.h under kDeltaLit for the paths idx at the points `at`: four draws;
        (ok, dir, maxt, Ld, pdf_em, pdf_bsdf).  A delta sample's densities are (1, 0): the balance heuristic gives exactly 1."""
        k = idx.shape[0]
        xs = np.stack([draw(idx), draw(idx), draw(idx), draw(idx)], -1)
        ok = np.zeros(k, bool)
        from_delta[idx] = False
        dirs, hi, Ld = np.zeros((k, 3), F), np.zeros(k, F), np.zeros((k, 3), F)
        pdf_em, pdf_bsdf = np.zeros(k, F), np.zeros(k, F)
        ei = np.minimum((xs[:, 0] * F(nL)).astype(np.int64), nL - 1)
        pdfPick = one / F(nL)
        is_env = (ei == env_index) if ENV else np.zeros(k, bool)
        is_area = ~is_env & (ei < nE)
        is_delta = ~is_env & ~is_area
        events["env_pick_shifted"][idx[is_env]] += 1
        # ---- the environment: a direction from xi, xiT unused
        e = np.nonzero(is_env)[0]
        if e.size:
            assert not med
            dr, le, pdfW, _ = env.sample(xs[e, 2:4])
            wo = _to_local(frame[0][e], frame[1][e], frame[2][e], dr)
            f, pb = surface_bsdf(mesh[e], alb[e], wi[e], wo)
            good = (pdfW > 0) & ~_is_zero(f)
            pe = pdfW * pdfPick
            with np.errstate(all="ignore"):
                ld = ((f * le) * (wo[:, 2] / pe)[:, None]).astype(F)
            ok[e], dirs[e], hi[e], Ld[e], pdf_em[e], pdf_bsdf[e] = good, dr, F(np.inf), ld, pe, pb
        # ---- an area light or a delta light: one tail (cosY = 1, pdfA = pdfPick; the sun: dist2 = 1)
        a = np.nonzero(~is_env)[0]
        if a.size:
            ka = a.size
            delta = is_delta[a]
            dr, dist, dist2 = np.zeros((ka, 3), F), np.zeros(ka, F), np.zeros(ka, F)
            cosY, pdfA, mx = np.ones(ka, F), np.full(ka, pdfPick, F), np.zeros(ka, F)
            rad, good = np.zeros((ka, 3), F), np.zeros(ka, bool)
            q = np.nonzero(delta)[0]
            if q.size:
                li = np.clip(ei[a[q]] - nE, 0, nD - 1)
                g_, dr[q], mx[q], rad[q], dist2[q], dist[q], band = incident_full(LT, li, at[a[q]], mutate)
                good[q] = g_
                gq = idx[a[q]]
                for t_, name in ((POINT, "pick_point"), (SPOT, "pick_spot"), (DIRECTIONAL, "pick_directional")):
                    events[name][gq[LT.type[li] == t_]] += 1
                events["spot_in_band"][gq[band]] += 1
                events["delta_outside_cone"][gq[~g_ & (LT.type[li] == SPOT) & (dist2[q] != 0)]] += 1
                if med:
                    events["delta_at_medium_vertex"][gq] += 1
            q = np.nonzero(~delta)[0]
            if q.size:
                lm, tri, p = light_cases.pick_reference(scene, pick_tables, xs[a[q]])
                su = np.sqrt(one - xs[a[q], 2])
                alpha = one - su
                beta = xs[a[q], 3] * su
                gamma = (one - alpha) - beta
                nrm = np.zeros((q.size, 3), F)
                for mi in np.unique(lm):
                    sel = lm == mi
                    m = meshes[int(mi)]
                    vi = m.indices[tri[sel]].astype(np.int64)
                    if m.normals is not None:
                        nv = m.normals[vi].astype(F)
                        nrm[sel] = _normalized((alpha[sel, None] * nv[:, 0] + beta[sel, None] * nv[:, 1]) + gamma[sel, None] * nv[:, 2])
                    else:
                        v = m.positions[vi].astype(F)
                        nrm[sel] = _normalized(cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(F))
                dvec = (p - at[a[q]]).astype(F)
                dist2[q] = dot(dvec, dvec)
                dist[q] = np.sqrt(dist2[q])
                with np.errstate(all="ignore"):
                    dr[q] = (dvec / dist[q][:, None]).astype(F)
                cosY[q] = dot(nrm, -dr[q])
                good[q] = cosY[q] > 0
                mx[q] = dist[q] - KEPS
                pdfA[q] = inv_area[lm] * pdfPick
                rad[q] = rad_of[lm]
            with np.errstate(all="ignore"):
                tr = mr.transmittance(medium, dist) if MEDIUM else None
                pe = np.where(delta, one, (pdfA * dist2) / cosY).astype(F)
                if med:
                    ph = mr.hg_eval(medium, dot(di[a], dr))
                    pb = np.where(delta, zero, ph).astype(F)
                    ld = (ph[:, None] * rad) * (cosY / (dist2 * pdfA))[:, None]
                    use_tr = np.ones(ka, bool)
                else:
                    wo = _to_local(frame[0][a], frame[1][a], frame[2][a], dr)
                    f, pb = surface_bsdf(mesh[a], alb[a], wi[a], wo)
                    events["delta_bsdf_zero"][idx[a[delta & good & _is_zero(f)]]] += 1
                    good = good & ~_is_zero(f)
                    if mutate == "mis_weight_from_quotient":      # the densities a light with an area would have: pdfPick dist2, the BSDF's
                        pe = np.where(delta, pdfA * dist2, pe).astype(F)
                    else:
                        pb = np.where(delta, zero, pb).astype(F)
                    ld = (f * rad) * ((wo[:, 2] * cosY) / (dist2 * pdfA))[:, None]
                    use_tr = np.full(ka, MEDIUM)
                if MEDIUM:
                    if mutate == "no_tr_on_delta":
                        use_tr = use_tr & ~delta
                    ld = np.where(use_tr[:, None], ld * tr[:, None], ld)
                    events["delta_tr"][idx[a[delta & good]]] += 1
            gd = idx[a[delta & good]]
            from_delta[gd] = True
            events["delta_black_shadow"][idx[a[delta & good & _is_zero(rad)]]] += 1
            events["hard_edge_lit"][idx[a[delta & good & hard[np.clip(ei[a] - nE, 0, nD - 1)]]]] += 1
            events["delta_empty_interval"][idx[a[delta & good & (mx < KEPS)]]] += 1
            if med and LENS:
                events["delta_medium_lens"][gd] += 1
            if MIS:
                events["delta_sample_mis"][gd] += 1
            events["delta_shadow"][idx[a[delta & good & np.isfinite(mx)]]] += 1
            ok[a], dirs[a], hi[a], Ld[a], pdf_em[a], pdf_bsdf[a] = good, dr, mx, ld.astype(F), pe, pb
        return ok, dirs, hi, Ld, pdf_em, pdf_bsdf

    for _ in range(max_vertices):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        its = query(idx, o[idx], d[idx], mint[idx], maxt[idx], False)
        n_closest += idx.size
        events["vertices"][idx] += 1
        found = its["mesh"] != NO_HIT
        di = d[idx]
        k = idx.size
        if MEDIUM:
            s = mr.distance(medium, draw(idx))
            med = ~found | (s < its["t"])
        else:
            med = np.zeros(k, bool)
        origin, cont = np.zeros((k, 3), F), np.zeros((k, 3), F)
        ends = np.zeros(k, bool)                   # the path ends at this vertex, before any shadow ray
        dead = np.zeros(k, bool)                   # no continuation (after the shadow ray, if any)
        shadow = np.zeros(k, bool)
        sh_dir, sh_maxt, Ld = np.zeros((k, 3), F), np.zeros(k, F), np.zeros((k, 3), F)
        Tn, pm = T[idx].copy(), pdf_mat[idx].copy()

        # ---------------- the ray left the scene: the environment, weighted as an emitter hit is
        esc = np.nonzero(~found & ~med)[0]
        ends[esc] = True
        if ENV and esc.size:
            g = idx[esc]
            weighted = prev[g] != 2
            le, pdfW, _ = env.eval(di[esc])
            if MIS:
                pdfEm = pdfW * (one / F(nL))
                w = np.where(weighted, _mis(pm[esc], pdfEm), one).astype(F)
            else:
                w = np.where(weighted, zero, one).astype(F)      # (path_ems counts it at the vertex before)
            add = w > 0
            L[g[add]] = (L[g[add]] + (Tn[esc][add] * le[add]) * w[add][:, None]).astype(F)

        # ---------------- medium vertices
        a = np.nonzero(med)[0]
        if a.size:
            ga = idx[a]
            origin[a] = (o[ga] + di[a] * s[a][:, None]).astype(F)
            Tn[a] = Tn[a] * medium.albedo[None, :]
            black = _is_zero(Tn[a])
            ends[a[black]] = True
            go = a[~black]
            rr = go[depth[idx[go]] >= 3]
            if rr.size:
                keep, Tn[rr] = roulette(idx[rr], Tn[rr])
                ends[rr[~keep]] = True
            go = go[~ends[go]]
            if go.size:
                ok, dirs, hi, ld, pdf_em, pdf_ph = sample_direct(idx[go], origin[go], True, di=di[go])
                w = _mis(pdf_em, pdf_ph) if MIS else np.ones(go.size, F)
                val = ((Tn[go] * ld) * w[:, None]).astype(F)
                g_ok = go[ok]
                shadow[g_ok] = True
                sh_dir[g_ok], sh_maxt[g_ok], Ld[g_ok] = dirs[ok], hi[ok], val[ok]
                xi = np.stack([draw(idx[go]), draw(idx[go])], -1)
                wo, pdf = mr.hg_sample(medium, di[go], xi)
                cont[go] = wo
                pm[go] = pdf if MIS else zero
                prev[idx[go]] = 1
                depth[idx[go]] += 1

        # ---------------- surface vertices
        b = np.nonzero(found & ~med)[0]
        if b.size:
            gb = idx[b]
            mesh = its["mesh"][b].astype(np.int64)
            fs, ft, fn = its["sh_s"][b].astype(F), its["sh_t"][b].astype(F), its["sh_n"][b].astype(F)
            origin[b] = its["p"][b]
            wi = _to_local(fs, ft, fn, -di[b])
            cosY = wi[:, 2]                                                # dot(ns, -d)
            front = cosY > 0
            em = is_em[mesh]
            alb = albedo_of[mesh].copy()
            for mi in np.unique(mesh[textured[mesh]]):
                sel = mesh == mi
                alb[sel] = texture_ref.lookup(scene.textures[meshes[int(mi)].albedo_texture], its["uv"][b][sel])
            # weight of emission reached by BSDF / phase sampling
            wMat = np.ones(b.size, F)
            weighted = prev[gb] != 2
            if not MIS:
                wMat[weighted] = zero
            else:
                tt = its["t"][b].astype(F)
                count = (nL - nD) if mutate == "emitter_hit_pdf_without_lights_in_count" else nL
                with np.errstate(all="ignore"):
                    pdfA = inv_area[mesh] / F(max(count, 1))
                    pdfEm = np.where(front, ((pdfA * tt) * tt) / cosY, zero).astype(F)
                sel = weighted & em
                wMat[sel] = _mis(pm[b], pdfEm)[sel]
                events["emitter_hit_lights_count"][gb[sel & front]] += 1
            add = em & (wMat > 0)
            le = np.where(front[:, None], rad_of[mesh], zero).astype(F)
            Lb = L[gb]
            Lb[add] = (Lb[add] + (Tn[b][add] * le[add]) * wMat[add][:, None]).astype(F)
            L[gb] = Lb
            rr = b[depth[gb] >= 3]
            if rr.size:
                keep, Tn[rr] = roulette(idx[rr], Tn[rr])
                ends[rr[~keep]] = True
            live = ~ends[b]
            go = b[live]
            mesh, fs, ft, fn, wi, alb = mesh[live], fs[live], ft[live], fn[live], wi[live], alb[live]
            bt = btype[mesh]
            nee = (bt == 0) | (bt == 3)      # bsdf_is_diffuse: never mirror or glass
            if nee.any():
                q = np.nonzero(nee)[0]
                gq = go[q]
                ok, dirs, hi, ld, pdf_em, pdf_bsdf = sample_direct(idx[gq], origin[gq], False, frame=(fs[q], ft[q], fn[q]), wi=wi[q], mesh=mesh[q], alb=alb[q])
                w = _mis(pdf_em, pdf_bsdf) if MIS else np.ones(q.size, F)
                val = ((Tn[gq] * ld) * w[:, None]).astype(F)
                g_ok = gq[ok]
                shadow[g_ok] = True
                sh_dir[g_ok], sh_maxt[g_ok], Ld[g_ok] = dirs[ok], hi[ok], val[ok]
            if go.size:
                xi = np.stack([draw(idx[go]), draw(idx[go])], -1)
                wo, f = np.zeros((go.size, 3), F), np.zeros((go.size, 3), F)
                e, meas, pdf = np.ones(go.size, F), np.zeros(go.size, np.int64), np.zeros(go.size, F)
                for mi in np.unique(mesh):
                    sel = mesh == mi
                    bs = meshes[int(mi)].bsdf
                    if textured[mi]:                                       # src/diffuse.cpp with the hit's albedo
                        up = wi[sel, 2] > 0
                        w_ = Oracle.warp("cosine_hemisphere", xi[sel])
                        wo[sel] = np.where(up[:, None], w_, zero)
                        f[sel] = np.where(up[:, None], alb[sel], zero)
                        meas[sel] = np.where(up, 1, 0)
                        pdf[sel] = np.where(up & (w_[:, 2] > 0), KINVPI * w_[:, 2], zero)
                    else:
                        wo[sel], f[sel], e[sel], m_ = Oracle.bsdf_sample(bs, wi[sel], xi[sel])
                        meas[sel] = m_
                        pdf[sel] = Oracle.bsdf_pdf(bs, wi[sel], wo[sel])
                dd = _is_zero(f)                                           # bsdf_sample returned zero: no continuation
                dead[go[dd]] = True
                g2, k2 = go[~dd], ~dd
                Tn[g2] = Tn[g2] * f[k2]
                eta[idx[g2]] = eta[idx[g2]] * e[k2]
                cont[g2] = to_world(fs[k2], ft[k2], fn[k2], wo[k2])
                prev[idx[g2]] = meas[k2]
                pm[g2] = np.where(meas[k2] != 2, pdf[k2], zero) if MIS else zero
                depth[idx[g2]] += 1

        # ---------------- the shadow rays, then what goes on
        sh = np.nonzero(shadow & ~ends)[0]
        if sh.size:
            ans = query(idx[sh], origin[sh], sh_dir[sh], np.full(sh.size, KEPS, F), sh_maxt[sh], True)
            n_shadow += sh.size
            lit = ans["mesh"] == NO_HIT
            dark = idx[sh[~lit]]
            events["delta_occluded"][dark[from_delta[dark]]] += 1
            g = idx[sh[lit]]
            L[g] = (L[g] + Ld[sh[lit]]).astype(F)
        T[idx], pdf_mat[idx] = Tn, pm
        stop = ends | dead
        alive[idx[stop]] = False
        go = ~stop
        o[idx[go]], d[idx[go]] = origin[go], cont[go]
        mint[idx[go]], maxt[idx[go]] = KEPS, F(np.inf)
    assert not alive.any(), f"{int(alive.sum())} paths still alive after {max_vertices} vertices"
    assert np.isfinite(L).all()
    assert L.dtype == F
    return L, n_closest, n_shadow, events
