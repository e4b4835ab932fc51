"""Li of path_mats / path_ems / path_mis restated in numpy for EVERY material, with or without a homogeneous medium or an
environment map: the state machine of rt_path.h (path_on_closest, sample_direct) and of include/nori_hip.h ("In Li ..." under the
environment's and the medium's sections), vectorised over the paths, float32, every operation in the order the code states it.

Nothing here comes from the device under test.  Closest-hit and shadow answers are the CPU oracle's (backend.intersect), the BSDFs
are the oracle's (Oracle.bsdf_sample / eval / pdf, once per mesh BSDF on the rows that hit that mesh), the emitter tables are
those scene_prep.cpp makes on the host (Emu.emitter_tables), the pick is light_cases.pick_reference, fog steps are medium_ref's
with the pinned log / exp / sincos, sky steps are envmap_ref.EnvRef's, a textured albedo is texture_ref.lookup at the hit's uv.

walk() also counts, per path, the events the branches under test are taken at (EVENTS), and `mutate` names ONE deliberate
departure from the specification, applied here only: tests/test_path_ref_cpu.py shows that each departure changes the radiance of
paths the GPU tests render, so a device that took the branch wrongly would fail their bitwise comparison."""
from __future__ import annotations

import numpy as np

from tests import medium_ref as mr
from tests.medium_ref import F, KEPS, KINVPI, NO_HIT, cross, dot, to_world

DRAWS_PER_VERTEX = 8      # distance 1, Russian roulette 1, emitter 4, BSDF / phase 2
MAX_VERTICES = 64

EVENTS = (
    "rr_eta",                          # roulette decisions taken with eta != 1
    "medium_vertex_prev_discrete",     # medium vertices reached while prev_measure == 2 (the camera ray's included)
    "medium_vertex_after_specular",    # ... of them those after a mirror / glass bounce (depth > 0)
    "medium_vertex_inside_glass",      # medium vertices on a ray that a dielectric surface sent to its inner side (wo.z < 0)
    "env_escape_after_discrete",       # escapes to the environment after a discrete bounce: unweighted under every integrator
    "env_escape_weighted",             # escapes after a bounce that was not discrete (weight 0 under path_ems, MIS under path_mis)
    "emitter_hit_env_count",           # emitter hits whose MIS density divides by n_emitters + 1
    "nee_microfacet_area",             # emitter samples at microfacet surfaces that picked an area light
    "nee_microfacet_env",              # ... that picked the environment
    "nee_textured",                    # emitter samples at textured surfaces
    "hit_vertex_normals",              # surface vertices on meshes with vertex normals
    "pick_light_normals",              # picks of a light with vertex normals
    "shadow_tr_surface",               # shadow rays of a surface vertex whose Ld was multiplied by the transmittance
    # the branches tests/path_fuzz.py's rounds reach (FUZZ_EVENTS); the hand-made cases of tests/path_cases.py reach none but,
    # by accident of their geometry, emitter_hit_backface
    "textured_vertex_mesh_uv",         # textured vertices on meshes with texcoords: hit_uv interpolates the corners' (rt_trace.h)
    "nee_env_only",                    # emitter samples where the environment is the only light (n_emitters = 0)
    "emitter_hit_backface",            # emitter hits with dot(ns, -d) <= 0: no emission
    "emitter_vertex_reflects",         # a path continues from a light whose BSDF reflects (albedo > 0)
    "medium_vertex_lens",              # medium vertices of frames seen through a thin lens
)
FUZZ_EVENTS = EVENTS[-5:]
MUTATIONS = {      # name -> the counter that is non-zero on every path the departure can change
    "roulette_without_eta": "rr_eta",
    "emitter_hit_pdf_without_env_in_count": "emitter_hit_env_count",
    "medium_vertex_keeps_discrete": "medium_vertex_prev_discrete",
    "env_escape_weighted_after_discrete": "env_escape_after_discrete",
    "no_tr_at_surface_nee": "shadow_tr_surface",
    "texture_not_in_nee": "nee_textured",
    "no_nee_at_microfacet": ("nee_microfacet_area", "nee_microfacet_env"),
    "geometric_normal_on_emitters": "pick_light_normals",
    # FUZZ_MUTATIONS: shown on tests/path_fuzz.py's rounds
    "barycentric_uv_on_meshes_with_texcoords": "textured_vertex_mesh_uv",      # hit_uv returns (u, v) as if the mesh had no texcoords
    "texcoords_of_rotated_corners": "textured_vertex_mesh_uv",                 # ... interpolates the uv of the vertices (1, 2, 0)
    "env_pick_divides_by_n_emitters": "nee_env_only",      # the light count without the + 1 where the environment is the only
                                                           # light: 0, sample_direct's early-out, no emitter sample
    "emission_from_both_sides": "emitter_hit_backface",
    "paths_end_at_emitters": "emitter_vertex_reflects",
}
FUZZ_MUTATIONS = tuple(MUTATIONS)[-5:]
UV_MUTATIONS = FUZZ_MUTATIONS[:2]

def emitter_tables(scene):
    """Emu(scene).emitter_tables(): the tables scene_prep.cpp makes on the host"""
    from tests.backends import Emu
    e = Emu(scene)
    tables = e.emitter_tables()
    e.close()
    return tables


def as_medium(m):
    return None if m is None else m if isinstance(m, mr.Medium) else mr.Medium(m.sigma_t, m.albedo, m.g)


def as_env(e):
    from tests.envmap_ref import EnvRef
    return None if e is None else e if isinstance(e, EnvRef) else EnvRef(e.texels, e.scale, e.to_world)


def _normalized(v):
    """normalized() of rt_types.h: a / sqrt(dot(a, a)) where that is > 0"""
    z = dot(v, v)
    with np.errstate(all="ignore"):
        return np.where((z > 0)[:, None], v / np.sqrt(z)[:, None], v).astype(F)


def _to_local(s, t, n, v):
    return np.stack([dot(v, s), dot(v, t), dot(v, n)], -1).astype(F)


def _is_zero(c):
    return (c == 0).all(axis=1)


def _mis(a, b):
    """a / (a + b) where a + b > 0, else 0"""
    with np.errstate(all="ignore"):
        return np.where(a + b > 0, a / (a + b), F(0.0)).astype(F)


def walk(backend, scene, integrator, rays, floats, medium=None, env=None, max_vertices=MAX_VERTICES, mutate=None):
    """(L [n, 3] float32, n_closest, n_shadow, events): Li of `rays` in `scene` under path_mats / path_ems / path_mis, the scene
    filled with `medium` (scene.Medium or medium_ref.Medium) or lit by `env` (scene.Environment or envmap_ref.EnvRef), never both.
    floats[k]: the numbers path k draws, in order, from its first vertex on (DRAWS_PER_VERTEX per vertex at most).  backend answers
    the ray queries (the scene's Oracle).  events: a dict of per-path int64 counters, one per name of EVENTS, and "vertices".  Every path must end
    within max_vertices (asserted) and L is finite (asserted)."""
    from tests import light_cases, texture_ref
    from tests.backends import Oracle
    assert integrator in ("path_mats", "path_ems", "path_mis")
    assert mutate is None or mutate in MUTATIONS, mutate
    medium, env = as_medium(medium), as_env(env)
    assert medium is None or env is None
    EMS, MIS = integrator != "path_mats", integrator == "path_mis"
    MEDIUM, ENV = medium is not None, env is not None
    LENS = scene.camera.aperture_radius > 0
    n = rays.shape[0]
    floats = np.ascontiguousarray(floats, F)
    assert floats.shape[0] == n and floats.shape[1] >= max_vertices * DRAWS_PER_VERTEX
    one, zero = F(1.0), F(0.0)

    meshes = scene.meshes
    tables = emitter_tables(scene)
    nE = sum(1 for m in meshes if m.radiance is not None)
    assert tables["n_emitters"] == nE
    nL = nE + 1 if ENV else nE                     # the lights: the environment is the last
    pick_tables = dict(tables, n_emitters=nL, emitters=np.concatenate([tables["emitters"], np.zeros(nL - nE, np.uint32)]))
    inv_area = tables["inv_area"].astype(F)
    btype = np.array([{"diffuse": 0, "mirror": 1, "dielectric": 2, "microfacet": 3}[m.bsdf.type] for m in meshes])
    textured = np.array([m.albedo_texture is not None for m in meshes])
    assert not (textured & (btype != 0)).any()
    has_normals = np.array([m.normals is not None for m in meshes])
    has_uv = np.array([m.texcoords is not None for m in meshes])
    reflects = np.array([m.radiance is not None and any(x > 0 for x in m.bsdf.albedo) for m in meshes])
    plain = None      # (the two uv departures need the hit's barycentrics: the same scene without texcoords answers with them)
    if mutate in UV_MUTATIONS:
        import dataclasses
        plain = Oracle(dataclasses.replace(scene, meshes=[dataclasses.replace(m, texcoords=None) for m in meshes]), use_bvh=True)
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
    inside = np.zeros(n, bool)                     # (for the counters only: the current ray left a dielectric surface inwards)
    n_closest = n_shadow = 0
    events = {k: np.zeros(n, np.int64) for k in EVENTS + ("vertices",)}      # (vertices: the closest-hit answers a path consumed)

    def draw(idx):
        v = floats[idx, cur[idx]]
        cur[idx] += 1
        return v

    def query(idx, org, dirs, lo, hi, shadow):
        q = np.zeros(idx.shape[0], rays.dtype)
        q["o"], q["d"], q["mint"], q["maxt"] = org, dirs, lo, hi
        return backend.intersect(q, shadow=shadow)

    def rays_of(g):
        q = np.zeros(g.shape[0], rays.dtype)
        q["o"], q["d"], q["mint"], q["maxt"] = o[g], d[g], mint[g], maxt[g]
        return q

    def roulette(idx, Tn):
        """Russian roulette of the paths idx (all at depth >= 3) on their throughputs Tn: (kept, Tn / p)"""
        e = eta[idx]
        events["rr_eta"][idx[e != 1]] += 1
        m3 = np.maximum(Tn[:, 0], np.maximum(Tn[:, 1], Tn[:, 2]))
        p = np.minimum(m3 if mutate == "roulette_without_eta" else (m3 * e) * e, F(0.99))
        keep = draw(idx) < p
        with np.errstate(all="ignore"):
            return keep, (Tn / p[:, None]).astype(F)

    def surface_bsdf(mesh, alb, wi, wo, use_texture=True):
        """(bsdf_eval, bsdf_pdf) of the rows' mesh BSDFs; a textured diffuse mesh's with the rows' albedo"""
        f, pdf = np.zeros((mesh.shape[0], 3), F), np.zeros(mesh.shape[0], F)
        for mi in np.unique(mesh):
            sel = mesh == mi
            b = meshes[int(mi)].bsdf
            if textured[mi] and use_texture:
                up = (wi[sel, 2] > 0) & (wo[sel, 2] > 0)
                f[sel] = np.where(up[:, None], alb[sel] * KINVPI, zero)
                pdf[sel] = np.where(up, KINVPI * wo[sel, 2], zero)
            else:
                f[sel], pdf[sel] = Oracle.bsdf_eval(b, wi[sel], wo[sel]), Oracle.bsdf_pdf(b, wi[sel], wo[sel])
        return f, pdf

    def sample_direct(idx, at, med, di=None, frame=None, wi=None, mesh=None, alb=None):
        """sample_direct of rt_path.h for the paths idx at the points `at`: four draws; (ok, dir, maxt, Ld, pdf_em, pdf_bsdf).
        med: medium vertices (di: the direction of travel); else surface vertices (frame = (s, t, n), wi, mesh, alb)."""
        k = idx.shape[0]
        xs = np.stack([draw(idx), draw(idx), draw(idx), draw(idx)], -1)
        ok = np.zeros(k, bool)
        dirs, hi, Ld = np.zeros((k, 3), F), np.zeros(k, F), np.zeros((k, 3), F)
        pdf_em, pdf_bsdf = np.zeros(k, F), np.zeros(k, F)
        if ENV and nE == 0:
            events["nee_env_only"][idx] += 1
        if nL == 0 or (mutate == "env_pick_divides_by_n_emitters" and nE == 0):
            return ok, dirs, hi, Ld, pdf_em, pdf_bsdf
        ei = np.minimum((xs[:, 0] * F(nL)).astype(np.int64), nL - 1)
        pdfPick = one / F(nL)
        is_env = (ei == nE) if ENV else np.zeros(k, bool)
        if not med:
            mf = btype[mesh] == 3
            events["nee_microfacet_area"][idx[mf & ~is_env]] += 1
            events["nee_microfacet_env"][idx[mf & is_env]] += 1
            events["nee_textured"][idx[textured[mesh]]] += 1
            nee_alb = albedo_of[mesh] if mutate == "texture_not_in_nee" else alb
        # ---- the environment: a direction from xi, xiT unused
        e = np.nonzero(is_env)[0]
        if e.size:
            assert not med
            dr, le, pdfW, _ = env.sample(xs[e, 2:4])
            wo = _to_local(frame[0][e], frame[1][e], frame[2][e], dr)
            f, pb = surface_bsdf(mesh[e], nee_alb[e], wi[e], wo, mutate != "texture_not_in_nee")
            good = (pdfW > 0) & ~_is_zero(f)
            pe = pdfW * pdfPick
            with np.errstate(all="ignore"):
                ld = ((f * le) * (wo[:, 2] / pe)[:, None]).astype(F)
            ok[e], dirs[e], hi[e], Ld[e], pdf_em[e], pdf_bsdf[e] = good, dr, F(np.inf), ld, pe, pb
        # ---- an area light: uniform emitter, triangle by area, uniform barycentrics
        a = np.nonzero(~is_env)[0]
        if a.size:
            lm, tri, p = light_cases.pick_reference(scene, pick_tables, xs[a])
            su = np.sqrt(one - xs[a, 2])
            alpha = one - su
            beta = xs[a, 3] * su
            gamma = (one - alpha) - beta
            nrm = np.zeros((a.size, 3), F)
            for mi in np.unique(lm):
                sel = lm == mi
                m = meshes[int(mi)]
                vi = m.indices[tri[sel]].astype(np.int64)
                if m.normals is not None:
                    events["pick_light_normals"][idx[a[sel]]] += 1
                if m.normals is not None and mutate != "geometric_normal_on_emitters":
                    nv = m.normals[vi].astype(F)
                    nrm[sel] = _normalized((alpha[sel, None] * nv[:, 0] + beta[sel, None] * nv[:, 1]) + gamma[sel, None] * nv[:, 2])
                else:
                    v = m.positions[vi].astype(F)
                    nrm[sel] = _normalized(cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(F))
            dvec = (p - at[a]).astype(F)
            dist2 = dot(dvec, dvec)
            dist = np.sqrt(dist2)
            with np.errstate(all="ignore"):
                dr = (dvec / dist[:, None]).astype(F)
                cosY = dot(nrm, -dr)
                good = cosY > 0
                tr = mr.transmittance(medium, dist) if MEDIUM else None
                pdfA = inv_area[lm] * pdfPick
                pe = (pdfA * dist2) / cosY
                rad = rad_of[lm]
                if med:
                    ph = mr.hg_eval(medium, dot(di[a], dr))
                    pb = ph
                    ld = ((ph[:, None] * rad) * (cosY / (dist2 * pdfA))[:, None]) * tr[:, None]
                else:
                    wo = _to_local(frame[0][a], frame[1][a], frame[2][a], dr)
                    f, pb = surface_bsdf(mesh[a], nee_alb[a], wi[a], wo, mutate != "texture_not_in_nee")
                    good = good & ~_is_zero(f)
                    ld = (f * rad) * ((wo[:, 2] * cosY) / (dist2 * pdfA))[:, None]
                    if MEDIUM and mutate != "no_tr_at_surface_nee":
                        ld = ld * tr[:, None]
                    if MEDIUM:
                        events["shadow_tr_surface"][idx[a[good]]] += 1
            ok[a], dirs[a], hi[a], Ld[a], pdf_em[a], pdf_bsdf[a] = good, dr, dist - KEPS, ld.astype(F), pe, pb
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
        # what a vertex leaves behind for its paths (positions within idx)
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
            discrete = prev[g] == 2
            after = discrete & (depth[g] > 0)
            events["env_escape_after_discrete"][g[after]] += 1
            events["env_escape_weighted"][g[~discrete]] += 1
            if mutate == "env_escape_weighted_after_discrete":
                discrete = discrete & ~after
            weighted = ~discrete if EMS else np.zeros(esc.size, bool)
            le, pdfW, _ = env.eval(di[esc])
            w = np.ones(esc.size, F)
            if MIS:
                pdfEm = pdfW * (one / F(nE + 1))
                w = np.where(weighted, _mis(pm[esc], pdfEm), one).astype(F)
            elif EMS:
                w = np.where(weighted, zero, one).astype(F)      # (path_ems counts it at the vertex before)
            add = w > 0
            L[g[add]] = (L[g[add]] + (Tn[esc][add] * le[add]) * w[add][:, None]).astype(F)

        # ---------------- medium vertices
        a = np.nonzero(med)[0]
        if a.size:
            ga = idx[a]
            origin[a] = (o[ga] + di[a] * s[a][:, None]).astype(F)
            was_discrete = prev[ga] == 2
            events["medium_vertex_prev_discrete"][ga[was_discrete]] += 1
            events["medium_vertex_after_specular"][ga[was_discrete & (depth[ga] > 0)]] += 1
            events["medium_vertex_inside_glass"][ga[inside[ga]]] += 1
            if LENS:
                events["medium_vertex_lens"][ga] += 1
            Tn[a] = Tn[a] * medium.albedo[None, :]
            black = _is_zero(Tn[a])
            ends[a[black]] = True
            go = a[~black]
            rr = go[depth[idx[go]] >= 3]
            if rr.size:
                keep, Tn[rr] = roulette(idx[rr], Tn[rr])
                ends[rr[~keep]] = True
            go = go[~ends[go]]
            if EMS and go.size:
                ok, dirs, hi, ld, pdf_em, pdf_ph = sample_direct(idx[go], origin[go], True, di=di[go])
                w = _mis(pdf_em, pdf_ph) if MIS else np.ones(go.size, F)
                val = ((Tn[go] * ld) * w[:, None]).astype(F)
                g_ok = go[ok]
                shadow[g_ok] = True
                sh_dir[g_ok], sh_maxt[g_ok], Ld[g_ok] = dirs[ok], hi[ok], val[ok]
            if go.size:
                xi = np.stack([draw(idx[go]), draw(idx[go])], -1)
                wo, pdf = mr.hg_sample(medium, di[go], xi)
                cont[go] = wo
                pm[go] = pdf if MIS else zero
                if mutate != "medium_vertex_keeps_discrete":
                    prev[idx[go]] = 1
                depth[idx[go]] += 1

        # ---------------- surface vertices
        b = np.nonzero(found & ~med)[0]
        if b.size:
            gb = idx[b]
            mesh = its["mesh"][b].astype(np.int64)
            fs, ft, fn = its["sh_s"][b].astype(F), its["sh_t"][b].astype(F), its["sh_n"][b].astype(F)
            origin[b] = its["p"][b]
            events["hit_vertex_normals"][gb[has_normals[mesh]]] += 1
            wi = _to_local(fs, ft, fn, -di[b])
            cosY = wi[:, 2]                                                # dot(ns, -d)
            front = cosY > 0
            em = is_em[mesh]
            alb = albedo_of[mesh].copy()
            for mi in np.unique(mesh[textured[mesh]]):                     # the albedo of bsdf_eval / pdf / sample and sample_direct alike
                sel = mesh == mi
                uv = its["uv"][b][sel]
                if has_uv[mi]:                                             # the oracle's interpolation is hit_uv's: oracle_scene.h, Accel::fill
                    events["textured_vertex_mesh_uv"][gb[sel]] += 1
                    if plain is not None:
                        bary = plain.intersect(rays_of(idx[b][sel]), shadow=False)
                        assert (bary["mesh"] == mi).all() and (bary["tri"] == its["tri"][b][sel]).all()
                        u, v = bary["uv"][:, 0], bary["uv"][:, 1]
                        uv = np.stack([u, v], 1)
                        if mutate == "texcoords_of_rotated_corners":
                            tc = meshes[int(mi)].texcoords[meshes[int(mi)].indices[its["tri"][b][sel]].astype(np.int64)][:, [1, 2, 0]]
                            b0 = one - (u + v)
                            uv = ((b0[:, None] * tc[:, 0] + u[:, None] * tc[:, 1]) + v[:, None] * tc[:, 2]).astype(F)
                alb[sel] = texture_ref.lookup(scene.textures[meshes[int(mi)].albedo_texture], uv)
            # weight of emission reached by BSDF / phase sampling
            wMat = np.ones(b.size, F)
            weighted = (prev[gb] != 2) if EMS else np.zeros(b.size, bool)
            if EMS and not MIS:
                wMat[weighted] = zero
            elif MIS:
                tt = its["t"][b].astype(F)
                count = nE if mutate == "emitter_hit_pdf_without_env_in_count" else nL
                with np.errstate(all="ignore"):
                    pdfA = inv_area[mesh] / F(max(count, 1))
                    pdfEm = np.where(front, ((pdfA * tt) * tt) / cosY, zero).astype(F)
                sel = weighted & em
                wMat[sel] = _mis(pm[b], pdfEm)[sel]
                if ENV:
                    events["emitter_hit_env_count"][gb[sel & front]] += 1
            add = em & (wMat > 0)
            events["emitter_hit_backface"][gb[em & ~front]] += 1
            le = rad_of[mesh] if mutate == "emission_from_both_sides" else np.where(front[:, None], rad_of[mesh], zero).astype(F)
            Lb = L[gb]
            Lb[add] = (Lb[add] + (Tn[b][add] * le[add]) * wMat[add][:, None]).astype(F)
            L[gb] = Lb
            if mutate == "paths_end_at_emitters":
                ends[b[em]] = True
            rr = b[depth[gb] >= 3]
            if rr.size:
                keep, Tn[rr] = roulette(idx[rr], Tn[rr])
                ends[rr[~keep]] = True
            live = ~ends[b]
            go = b[live]
            mesh, fs, ft, fn, wi, alb = mesh[live], fs[live], ft[live], fn[live], wi[live], alb[live]
            bt = btype[mesh]
            nee = (bt == 0) if mutate == "no_nee_at_microfacet" else ((bt == 0) | (bt == 3))      # bsdf_is_diffuse: never mirror or glass
            if EMS and nee.any():
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
                inside[idx[g2]] = (bt[k2] == 2) & (wo[k2][:, 2] < 0)
                pm[g2] = np.where(meas[k2] != 2, pdf[k2], zero) if MIS else zero
                depth[idx[g2]] += 1
                events["emitter_vertex_reflects"][idx[g2][reflects[mesh[k2]]]] += 1

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
    assert np.isfinite(L).all()
    assert L.dtype == F
    return L, n_closest, n_shadow, events
