"""The grid medium (include/nori_hip.h, "Grid medium") restated in numpy: float32, every operation in the order the header states
it, no contraction.  1 / x and a / b of numpy's float32 are the correctly rounded ones; log and exp are parameters, as in
tests/medium_ref.py -- by default the CPU restatement of the pinned functions, the GPU tests pass the device's own.

grid_walk() is the walk, vectorised over the rays; it also says which of its branches each ray took (BRANCHES), so that the tests can
show that their rays reach every one.  walk() restates Li as a whole for every material, area emitters and delta lights, in a scene
with a grid medium: the state machine of rt_path.h under kGridMedium.  Its surface and light pieces are path_ref's,
delta_lights_ref's and medium_ref's by import; nothing here comes from the device."""
from __future__ import annotations

import numpy as np

from tests import medium_ref as mr
from tests.medium_ref import F, KEPS, KINVPI, NO_HIT, cross, dot, to_world

PARALLEL = F(2.0 ** -40)
INF = F(np.inf)
DRAWS_PER_VERTEX = mr.DRAWS_PER_VERTEX
BRANCHES = ("miss", "enter_from_outside", "start_inside", "stop_at_tmax_inside", "tie_of_two", "tie_of_three", "parallel_inside",
            "parallel_outside", "zero_voxel_skipped", "event_in_last_voxel")
# deliberate departures: of the walk (the first two), of Li (the others)
MUTATIONS = ("accumulate_boundaries", "ties_z_first", "no_tr_on_emitter_samples", "tr_over_unclipped_distance", "medium_vertex_whenever_not_found")


class Grid:
    """rho (nz, ny, nx), the box, sigma_scale and what the host derives once, in float32; albedo and g as medium_ref.Medium"""

    def __init__(self, rho, bmin, bmax, sigma_scale, albedo=(1.0, 1.0, 1.0), g=0.0):
        self.rho = np.ascontiguousarray(rho, F)
        assert self.rho.ndim == 3
        self.n = np.array(self.rho.shape[::-1], np.int64)                      # (nx, ny, nz)
        self.bmin, self.bmax = np.asarray(bmin, F).reshape(3), np.asarray(bmax, F).reshape(3)
        ext = self.bmax - self.bmin
        self.cell = (ext / self.n.astype(F)).astype(F)
        self.inv_cell = (self.n.astype(F) / ext).astype(F)
        self.sigma_scale = F(sigma_scale)
        self.phase = mr.Medium(sigma_scale if sigma_scale > 0 else 1.0, albedo, g)
        self.albedo = self.phase.albedo


def as_grid(m):
    return m if isinstance(m, Grid) else Grid(m.rho, m.bmin, m.bmax, m.sigma_scale, m.albedo, m.g)


def grid_walk(g: Grid, o, d, tmax, tau_stop, mutate=None):
    """(tau, s, event, steps, branches) of n rays: the header's walk.  branches: name -> bool (n,)."""
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    tmax, tau_stop = np.broadcast_to(np.asarray(tmax, F), (n,)), np.broadcast_to(np.asarray(tau_stop, F), (n,))
    one, zero = F(1.0), F(0.0)
    br = {k: np.zeros(n, bool) for k in BRANCHES}
    par = np.abs(d) < PARALLEL
    with np.errstate(all="ignore"):
        inv = (one / np.where(par, one, d)).astype(F)
        step = np.where(par, 0, np.where(d > 0, 1, -1)).astype(np.int64)
        in_slab = (o >= g.bmin) & (o < g.bmax)
        miss = (par & ~in_slab).any(axis=1)
        br["parallel_outside"] = miss.copy()
        ta, tb = ((g.bmin - o) * inv).astype(F), ((g.bmax - o) * inv).astype(F)
        tn, tf = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
        t0, t1 = np.zeros(n, F), tmax.astype(F).copy()
        for a in range(3):
            t0 = np.where(~par[:, a] & (tn[:, a] > t0), tn[:, a], t0)
            t1 = np.where(~par[:, a] & (tf[:, a] < t1), tf[:, a], t1)
        miss = miss | par.all(axis=1) | ~(t0 < t1)
        p = np.where(par, o, (o + (d * t0[:, None]).astype(F)).astype(F))
        c = np.floor(((p - g.bmin) * g.inv_cell).astype(F))
    hi = (g.n - 1).astype(F)
    c = np.where(c >= 0, c, zero)
    c = np.where(c <= hi, c, hi)
    i = c.astype(np.int64)
    br["miss"] = miss & ~br["parallel_outside"]
    br["enter_from_outside"] = ~miss & (t0 > 0)
    br["start_inside"] = ~miss & (t0 == 0)
    br["parallel_inside"] = ~miss & par.any(axis=1)
    active = ~miss
    t_cur, tau = t0.copy(), np.zeros(n, F)
    s, event, steps = np.full(n, INF, F), np.zeros(n, bool), np.zeros(n, np.int32)
    acc = None      # (mutation) the crossings, accumulated
    cap = int(g.n.sum())
    for _ in range(cap):
        if not active.any():
            break
        with np.errstate(all="ignore"):
            k = i + (step > 0)
            plane = (g.bmin + (k.astype(F) * g.cell).astype(F)).astype(F)
            t = np.where(step == 0, INF, ((plane - o) * inv).astype(F)).astype(F)
            if mutate == "accumulate_boundaries":
                if acc is None:
                    acc = t.copy()
                t = acc
            if mutate == "ties_z_first":
                sz = (t[:, 2] <= t[:, 1]) & (t[:, 2] <= t[:, 0])
                sy = ~sz & (t[:, 1] <= t[:, 0])
                sx = ~sz & ~sy
            else:
                sx = (t[:, 0] <= t[:, 1]) & (t[:, 0] <= t[:, 2])
                sy = ~sx & (t[:, 1] <= t[:, 2])
                sz = ~sx & ~sy
            t_next = np.where(sx, t[:, 0], np.where(sy, t[:, 1], t[:, 2])).astype(F)
            t_end = np.where(t_next < t1, t_next, t1)
            ic = np.clip(i, 0, g.n - 1)
            sigma = (g.sigma_scale * g.rho[ic[:, 2], ic[:, 1], ic[:, 0]]).astype(F)
            ln = (t_end - t_cur).astype(F)
            tau_new = (tau + (sigma * np.where(ln > 0, ln, zero)).astype(F)).astype(F)
            steps[active] += 1
            ev = active & (sigma > 0) & (tau_new >= tau_stop)
            s_here = ((t_cur + ((tau_stop - tau).astype(F) / sigma).astype(F)).astype(F) + zero).astype(F)
        s[ev] = s_here[ev]
        event |= ev
        go = active & ~ev
        tau = np.where(go, tau_new, tau)
        cont = go & (t_next < t1)
        ties = (t == t_next[:, None]).sum(axis=1)
        br["tie_of_two"] |= cont & (ties == 2)
        br["tie_of_three"] |= cont & (ties == 3)
        br["zero_voxel_skipped"] |= go & (sigma == 0) & (ln > 0)
        br["stop_at_tmax_inside"] |= go & ~cont & (t1 == tmax) & np.isfinite(tmax)
        t_cur = np.where(cont & (t_next > t_cur), t_next, t_cur)
        mv = np.stack([sx, sy, sz], axis=1) & cont[:, None]
        i_new = i + np.where(mv, step, 0)
        inside = ((i_new >= 0) & (i_new < g.n)).all(axis=1)
        br["event_in_last_voxel"] |= ev & ~((i + np.where(np.stack([sx, sy, sz], axis=1), step, 0) >= 0) & (i + np.where(np.stack([sx, sy, sz], axis=1), step, 0) < g.n)).all(axis=1)
        if mutate == "accumulate_boundaries":
            with np.errstate(all="ignore"):
                acc = np.where(mv, (acc + (g.cell * np.abs(inv)).astype(F)).astype(F), acc)
        i = np.where(cont[:, None], i_new, i)
        active = cont & inside
    assert not active.any(), "a walk took more than nx + ny + nz trips"
    assert (steps <= cap).all()
    return tau, s, event, steps, br


def distance(g: Grid, o, d, tmax, xi, log=mr.default_log, mutate=None):
    """(s, event): the free flight xi selects; s is +inf where there is no event"""
    xi = np.asarray(xi, F)
    tau, s, ev, _, _ = grid_walk(g, o, d, tmax, (-log(F(1.0) - xi)).astype(F), mutate)
    return s, ev


def optical_depth(g: Grid, o, d, tmax, mutate=None):
    tau, _, _, steps, _ = grid_walk(g, o, d, tmax, INF, mutate)
    return tau, steps


def transmittance(g: Grid, o, d, dist, exp=mr.default_exp, mutate=None):
    return exp(-optical_depth(g, o, d, dist, mutate)[0]).astype(F)


# ------------------------------------------------------------------ Li, restated
def walk(backend, scene, integrator, rays, floats, grid=None, lights=None, log=mr.default_log, exp=mr.default_exp, max_vertices=64, mutate=None):
    """(L [n, 3] float32, n_closest, n_shadow, events: name -> count per path [n]): Li of `rays` in `scene` -- every material, area emitters, the delta
    lights `lights` (default scene.lights; path_ems / path_mis only) -- with the grid medium `grid` (default scene.medium), under
    path_mats / path_ems / path_mis.  floats[k]: the numbers path k draws, in order, from its first vertex on.  backend answers every
    closest-hit and shadow query."""
    from tests import delta_lights_ref as dl, light_cases, path_ref as pr, texture_ref
    from tests.backends import Oracle
    assert integrator in ("path_mats", "path_ems", "path_mis")
    assert mutate is None or mutate in MUTATIONS, mutate
    G = as_grid(scene.medium if grid is None else grid)
    wmut = mutate if mutate in ("accumulate_boundaries", "ties_z_first") else None
    EMS, MIS = integrator != "path_mats", integrator == "path_mis"
    lights = list(scene.lights if lights is None else lights)
    LT = dl.as_lights(lights) if lights else None
    nD = LT.n if lights else 0
    assert nD == 0 or EMS
    n = rays.shape[0]
    floats = np.ascontiguousarray(floats, F)
    assert floats.shape[0] == n and floats.shape[1] >= max_vertices * DRAWS_PER_VERTEX
    one, zero = F(1.0), F(0.0)
    meshes = scene.meshes
    tables = pr.emitter_tables(scene)
    nE = sum(1 for m in meshes if m.radiance is not None)
    nL = nE + nD
    pick_tables = dict(tables, n_emitters=nL, emitters=np.concatenate([tables["emitters"], np.zeros(nL - nE, np.uint32)]))
    inv_area = tables["inv_area"].astype(F)
    btype = np.array([{"diffuse": 0, "mirror": 1, "dielectric": 2, "microfacet": 3}[m.bsdf.type] for m in meshes])
    textured = np.array([m.albedo_texture is not None for m in meshes])
    albedo_of = np.array([m.bsdf.albedo for m in meshes], F)
    rad_of = np.array([m.radiance if m.radiance is not None else (0, 0, 0) for m in meshes], F)
    is_em = np.array([m.radiance is not None for m in meshes])

    o, d = rays["o"].astype(F).copy(), rays["d"].astype(F).copy()
    mint, maxt = rays["mint"].astype(F).copy(), rays["maxt"].astype(F).copy()
    T, L = np.ones((n, 3), F), np.zeros((n, 3), F)
    eta, pdf_mat = np.ones(n, F), np.zeros(n, F)
    prev = np.full(n, 2, np.int64)
    depth, cur = np.zeros(n, np.int64), np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    n_closest = n_shadow = 0
    events = {k: np.zeros(n, np.int64) for k in ("medium_vertex", "miss", "enter_from_outside", "start_inside", "left_scene_through_grid")}
    n_med = events["medium_vertex"]

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
            if textured[mi]:
                up = (wi[sel, 2] > 0) & (wo[sel, 2] > 0)
                f[sel] = np.where(up[:, None], alb[sel] * KINVPI, zero)
                pdf[sel] = np.where(up, KINVPI * wo[sel, 2], zero)
            else:
                b = meshes[int(mi)].bsdf
                f[sel], pdf[sel] = Oracle.bsdf_eval(b, wi[sel], wo[sel]), Oracle.bsdf_pdf(b, wi[sel], wo[sel])
        return f, pdf

    def sample_direct(idx, at, med, di=None, frame=None, wi=None, mesh=None, alb=None):
        """sample_direct of rt_path.h: four draws; (ok, dir, maxt, Ld, pdf_em, pdf_bsdf)"""
        k = idx.shape[0]
        xs = np.stack([draw(idx), draw(idx), draw(idx), draw(idx)], -1)
        ok = np.zeros(k, bool)
        dr, dist, dist2 = np.zeros((k, 3), F), np.zeros(k, F), np.zeros(k, F)
        cosY, mx = np.ones(k, F), np.zeros(k, F)
        rad = np.zeros((k, 3), F)
        if nL == 0:
            return ok, dr, mx, rad, np.zeros(k, F), np.zeros(k, F)
        pdfPick = one / F(nL)
        pdfA = np.full(k, pdfPick, F)
        ei = np.minimum((xs[:, 0] * F(nL)).astype(np.int64), nL - 1)
        delta = ei >= nE
        q = np.nonzero(delta)[0]
        if q.size:
            g_, dr[q], mx[q], rad[q], dist2[q], dist[q], _ = dl.incident_full(LT, np.clip(ei[q] - nE, 0, nD - 1), at[q])
            ok[q] = g_
        q = np.nonzero(~delta)[0]
        if q.size:
            lm, tri, p = light_cases.pick_reference(scene, pick_tables, xs[q])
            su = np.sqrt(one - xs[q, 2])
            alpha = one - su
            beta = xs[q, 3] * su
            gamma = (one - alpha) - beta
            nrm = np.zeros((q.size, 3), F)
            for mi in np.unique(lm):
                sel = lm == mi
                m = meshes[int(mi)]
                vi = m.indices[tri[sel]].astype(np.int64)
                if m.normals is not None:
                    nv = m.normals[vi].astype(F)
                    nrm[sel] = pr._normalized((alpha[sel, None] * nv[:, 0] + beta[sel, None] * nv[:, 1]) + gamma[sel, None] * nv[:, 2])
                else:
                    v = m.positions[vi].astype(F)
                    nrm[sel] = pr._normalized(cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(F))
            dvec = (p - at[q]).astype(F)
            dist2[q] = dot(dvec, dvec)
            dist[q] = np.sqrt(dist2[q])
            with np.errstate(all="ignore"):
                dr[q] = (dvec / dist[q][:, None]).astype(F)
            cosY[q] = dot(nrm, -dr[q])
            ok[q] = cosY[q] > 0
            mx[q] = dist[q] - KEPS
            pdfA[q] = inv_area[lm] * pdfPick
            rad[q] = rad_of[lm]
        with np.errstate(all="ignore"):
            if mutate == "no_tr_on_emitter_samples":
                tr = np.ones(k, F)
            else:
                tr = transmittance(G, at, dr, np.full(k, INF, F) if mutate == "tr_over_unclipped_distance" else dist, exp, wmut)
            pe = np.where(delta, one, (pdfA * dist2) / cosY).astype(F)
            if med:
                ph = mr.hg_eval(G.phase, dot(di, dr))
                pb = np.where(delta, zero, ph).astype(F)
                ld = ((ph[:, None] * rad) * (cosY / (dist2 * pdfA))[:, None]) * tr[:, None]
            else:
                wo = pr._to_local(frame[0], frame[1], frame[2], dr)
                f, pb = surface_bsdf(mesh, alb, wi, wo)
                ok = ok & ~pr._is_zero(f)
                pb = np.where(delta, zero, pb).astype(F)
                ld = ((f * rad) * ((wo[:, 2] * cosY) / (dist2 * pdfA))[:, None]) * tr[:, None]
        return ok, dr, mx, ld.astype(F), pe, pb

    for _ in range(max_vertices):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        its = query(idx, o[idx], d[idx], mint[idx], maxt[idx], False)
        n_closest += idx.size
        found = its["mesh"] != NO_HIT
        di = d[idx]
        k = idx.size
        _, s, ev, _, br = grid_walk(G, o[idx], di, np.where(found, its["t"].astype(F), INF), (-log(F(1.0) - draw(idx))).astype(F), wmut)
        for name in ("miss", "enter_from_outside", "start_inside"):
            events[name][idx[br[name]]] += 1
        med = ev & (~found | (s < its["t"]))
        if mutate == "medium_vertex_whenever_not_found":      # the homogeneous rule: a ray that leaves the scene always scatters
            med = med | ~found
        origin, cont = np.zeros((k, 3), F), np.zeros((k, 3), F)
        ends = np.zeros(k, bool)
        dead = np.zeros(k, bool)
        shadow = np.zeros(k, bool)
        sh_dir, sh_maxt, Ld = np.zeros((k, 3), F), np.zeros(k, F), np.zeros((k, 3), F)
        Tn, pm = T[idx].copy(), pdf_mat[idx].copy()
        ends[~found & ~med] = True      # the ray left the box and the scene: the path ends
        events["left_scene_through_grid"][idx[~found & ~med & ~br["miss"] & ~br["parallel_outside"]]] += 1

        # ---------------- medium vertices
        a = np.nonzero(med)[0]
        if a.size:
            ga = idx[a]
            n_med[ga] += 1
            sa = np.where(np.isfinite(s[a]), s[a], one)
            origin[a] = (o[ga] + di[a] * sa[:, None]).astype(F)
            Tn[a] = Tn[a] * G.albedo[None, :]
            black = pr._is_zero(Tn[a])
            ends[a[black]] = True
            go = a[~black]
            rr = go[depth[idx[go]] >= 3]
            if rr.size:
                keep, Tn[rr] = roulette(idx[rr], Tn[rr])
                ends[rr[~keep]] = True
            go = go[~ends[go]]
            if go.size:
                if EMS:
                    ok, dirs, hi, ld, pdf_em, pdf_ph = sample_direct(idx[go], origin[go], True, di=di[go])
                    w = pr._mis(pdf_em, pdf_ph) if MIS else np.ones(go.size, F)
                    val = ((Tn[go] * ld) * w[:, None]).astype(F)
                    g_ok = go[ok]
                    shadow[g_ok] = True
                    sh_dir[g_ok], sh_maxt[g_ok], Ld[g_ok] = dirs[ok], hi[ok], val[ok]
                xi = np.stack([draw(idx[go]), draw(idx[go])], -1)
                wo, pdf = mr.hg_sample(G.phase, di[go], xi)
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
            wi = pr._to_local(fs, ft, fn, -di[b])
            cosY = wi[:, 2]
            front = cosY > 0
            em = is_em[mesh]
            alb = albedo_of[mesh].copy()
            for mi in np.unique(mesh[textured[mesh]]):
                sel = mesh == mi
                alb[sel] = texture_ref.lookup(scene.textures[meshes[int(mi)].albedo_texture], its["uv"][b][sel])
            wMat = np.ones(b.size, F)
            weighted = prev[gb] != 2
            if EMS:
                if not MIS:
                    wMat[weighted] = zero
                else:
                    tt = its["t"][b].astype(F)
                    with np.errstate(all="ignore"):
                        pdfA = inv_area[mesh] / F(max(nL, 1))
                        pdfEm = np.where(front, ((pdfA * tt) * tt) / cosY, zero).astype(F)
                    sel = weighted & em
                    wMat[sel] = pr._mis(pm[b], pdfEm)[sel]
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
            nee = (bt == 0) | (bt == 3)
            if EMS and nee.any():
                q = np.nonzero(nee)[0]
                gq = go[q]
                ok, dirs, hi, ld, pdf_em, pdf_bsdf = sample_direct(idx[gq], origin[gq], False, frame=(fs[q], ft[q], fn[q]), wi=wi[q], mesh=mesh[q], alb=alb[q])
                w = pr._mis(pdf_em, pdf_bsdf) if MIS else np.ones(q.size, F)
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
                    if textured[mi]:
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
                dd = pr._is_zero(f)
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
            g = idx[sh[lit]]
            L[g] = (L[g] + Ld[sh[lit]]).astype(F)
        T[idx], pdf_mat[idx] = Tn, pm
        stop = ends | dead
        alive[idx[stop]] = False
        go = ~stop
        o[idx[go]], d[idx[go]] = origin[go], cont[go]
        mint[idx[go]], maxt[idx[go]] = KEPS, INF
    assert not alive.any(), f"{int(alive.sum())} paths still alive after {max_vertices} vertices"
    assert L.dtype == F
    return L, n_closest, n_shadow, events
