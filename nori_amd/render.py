"""`Renderer`: Python handle on a libnori_hip context (one GPU).

Thin glue over the C ABI of include/nori_hip.h: numpy in / numpy out for the
operator-level twins, torch CUDA tensors (device memory, streams) for the
frame buffer of the hot path.  No compute happens in Python.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi as capi
from ._capi import NoriError, ptr
from .scene import Bsdf, Scene


def _f32(a, shape_last=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape_last is not None:
        a = a.reshape(-1, shape_last)
    return a


def read_tree(call) -> dict:
    """The dict of Renderer.tree() from `call(root, counts, nodes, nodes32, grid, pairs)`, which follows nori_hip_debug_tree's convention:
    once with NULL arrays for the counts, once with arrays."""
    root, counts = C.c_int32(0), np.zeros(4, np.uint32)
    call(C.byref(root), ptr(counts), None, None, None, None)
    n_nodes, n_pairs, wide, q = (int(c) for c in counts)
    nodes, pairs = np.zeros((max(n_nodes, 1), 16), np.float32), np.zeros((max(n_pairs, 1), 24), np.float32)
    nodes32, grid = np.zeros((max(n_nodes, 1), 8), np.uint32), np.zeros(6, np.float32)
    call(C.byref(root), ptr(counts), ptr(nodes), ptr(nodes32), ptr(grid), ptr(pairs))
    assert (n_nodes, n_pairs, wide, q) == tuple(int(c) for c in counts)
    return {"root": int(root.value), "n_nodes": n_nodes, "n_pairs": n_pairs, "wide": wide, "records_32b": q, "nodes": nodes[:n_nodes],
            "pairs": pairs[:n_pairs], "nodes32": nodes32[:n_nodes] if q else None, "grid_mn": grid[:3].copy() if q else None,
            "grid_scale": grid[3:].copy() if q else None}


class Renderer:
    """Owns a `nori_hip_ctx`.  Mirrors Scene/Accel/Integrator of the reference:
    `upload` = Scene::addChild + activate, `build_accel` = Accel::build,
    `intersect` = Accel::rayIntersect, `li` = Integrator::Li, `render` =
    render() of src/main.cpp:58-119."""

    def __init__(self, device: int = 0):
        self._lib = capi.load_hip()
        h = C.c_void_p()
        rc = self._lib.nori_hip_create(int(device), C.byref(h))
        if rc != 0:
            msg = self._lib.nori_hip_last_error(None)
            raise NoriError(f"nori_hip_create({device}) failed: {capi.STATUS.get(rc, rc)}: "
                            f"{msg.decode() if msg else ''}")
        self._h = h
        self.device = int(device)
        self.scene: Optional[Scene] = None

    # -------------------------------------------------------------- plumbing
    def close(self):
        if getattr(self, "_h", None):
            self._lib.nori_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.nori_hip_last_error(self._h)
            raise NoriError(f"{what}: {capi.STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def excursions(self, reset: bool = False):
        """(rcp, div, sqrt operands outside the verified domain, fallbacks taken) -- libnori_hip_count.so only."""
        out = (C.c_ulonglong * 4)()
        self._check(self._lib.nori_hip_debug_excursions(self._h, out, int(reset)), "debug_excursions")
        return tuple(int(v) for v in out)

    # ------------------------------------------------------------ load time
    def upload(self, scene: Scene, build: bool = True, builder: int = 0):
        """builder: nori_accel_builder (include/nori_hip.h).  The default HERE is 0, NORI_ACCEL_HOST_SAH: the host's SAH builder, whose trees
        the suite's pinned expectations (depths, node counts, costs, which traversal-stack variant runs) were written for.  It is not
        what the library builds by default: that is 2, NORI_ACCEL_AUTO -- the device's builder (lbvh.hip; the host's only if the
        device's fails, silently: accel_info()["built_on_device"] tells) -- which the C++ host, bench.py, smoke() and the tools pass.
        The tests that carry the parity claims at full size run on both (tests/test_gpu_parity.py: BUILDERS); pass builder=2 to
        render through the tree a user of the library gets."""
        desc, keep = scene.c_desc()
        self._check(self._lib.nori_hip_upload_scene(self._h, C.byref(desc)), "upload_scene")
        del keep
        self.scene = scene
        if scene.camera.aperture_radius > 0:      # (the upload itself resets the context to the pinhole)
            self.set_lens(scene.camera.aperture_radius, scene.camera.focus_distance)
        if getattr(scene, "environment", None) is not None:      # (the upload itself resets the context to none)
            self.set_environment(scene.environment)
        if getattr(scene, "medium", None) is not None:
            self.set_medium(scene.medium)
        if getattr(scene, "lights", None):
            self.set_lights(scene.lights)
        if build:
            self.build_accel(builder)
        return self

    # ------------------------------------------------------------ delta lights
    def set_lights(self, lights):
        """The delta lights of the uploaded scene (include/nori_hip.h, "Delta lights"): a list of scene.Light, or None / an empty
        list for none -- the kernels and the bits of a context that never had lights.  Holds until the next upload."""
        from .scene import light_array
        lights = list(lights) if lights is not None else []
        self._check(self._lib.nori_hip_set_lights(self._h, len(lights), light_array(lights)), "set_lights")
        return self

    @property
    def lights(self):
        """The lights set, as the context stores them (directions normalised, unused fields zero): a list of scene.Light."""
        from .scene import Light
        n = C.c_uint32(0)
        self._check(self._lib.nori_hip_get_lights(self._h, 0, None, C.byref(n)), "get_lights")
        if n.value == 0:
            return []
        arr = (capi.LightDesc * n.value)()
        self._check(self._lib.nori_hip_get_lights(self._h, n.value, arr, C.byref(n)), "get_lights")
        return [Light.from_desc(arr[k]) for k in range(n.value)]

    def light_incident(self, light, p):
        """(dir (n, 3), maxt (n,), radiance (n, 3)): what the lights of the (n,) indices send towards the (n, 3) points, as the
        emitter sample computes it; zeros where there is no sample."""
        li = np.ascontiguousarray(light, dtype=np.uint32).reshape(-1)
        pts = _f32(p, 3)
        assert li.shape[0] == pts.shape[0]
        n = li.shape[0]
        d, hi, rad = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
        self._check(self._lib.nori_hip_light_incident(self._h, ptr(li), ptr(pts), n, ptr(d), ptr(hi), ptr(rad)), "light_incident")
        return d, hi, rad

    # ------------------------------------------------------------ homogeneous medium
    def set_medium(self, medium):
        """The homogeneous medium of the uploaded scene (include/nori_hip.h, "Homogeneous participating medium"): a scene.Medium, or
        None for no medium of either kind -- the kernels and the bits of a context that never had one.  Holds until the next upload.
        (A scene.GridMedium, which Scene.medium may hold instead, goes to set_grid_medium.)"""
        from .scene import GridMedium
        if isinstance(medium, GridMedium):
            return self.set_grid_medium(medium)
        d = medium.desc() if medium is not None else None
        self._check(self._lib.nori_hip_set_medium(self._h, C.byref(d) if d is not None else None), "set_medium")
        return self

    @property
    def medium(self):
        """The medium set, as the context stores it (g is 0 where |g| < 1e-3): a scene.Medium, or None."""
        from .scene import Medium
        d = capi.MediumDesc()
        rc = self._lib.nori_hip_get_medium(self._h, C.byref(d))
        if rc < 0:
            self._check(rc, "get_medium")
        return Medium(float(d.sigma_t), tuple(float(x) for x in d.albedo), float(d.g)) if rc == 1 else None

    def medium_distance(self, xi):
        """Free-flight distances -log(1 - xi) / sigma_t of the (n,) samples, as Li draws them."""
        x = np.ascontiguousarray(xi, dtype=np.float32).reshape(-1)
        s = np.zeros(x.shape[0], np.float32)
        self._check(self._lib.nori_hip_medium_distance(self._h, ptr(x), x.shape[0], ptr(s)), "medium_distance")
        return s

    def medium_transmittance(self, dist):
        """Tr(dist) = exp(-sigma_t dist) of the (n,) distances."""
        x = np.ascontiguousarray(dist, dtype=np.float32).reshape(-1)
        t = np.zeros(x.shape[0], np.float32)
        self._check(self._lib.nori_hip_medium_transmittance(self._h, ptr(x), x.shape[0], ptr(t)), "medium_transmittance")
        return t

    def phase_eval(self, d, wo):
        """The phase density HG(dot(d, wo)) of (n, 3) directions of travel d and scattered directions wo."""
        a, b = _f32(d, 3), _f32(wo, 3)
        assert a.shape == b.shape
        p = np.zeros(a.shape[0], np.float32)
        self._check(self._lib.nori_hip_phase_eval(self._h, ptr(a), ptr(b), a.shape[0], ptr(p)), "phase_eval")
        return p

    def phase_sample(self, d, xi):
        """(wo (n, 3), pdf (n,)): the phase sample the (n, 2) numbers xi select for the (n, 3) directions of travel d."""
        a, x = _f32(d, 3), _f32(xi, 2)
        assert a.shape[0] == x.shape[0]
        wo, p = np.zeros((a.shape[0], 3), np.float32), np.zeros(a.shape[0], np.float32)
        self._check(self._lib.nori_hip_phase_sample(self._h, ptr(a), ptr(x), a.shape[0], ptr(wo), ptr(p)), "phase_sample")
        return wo, p

    # ------------------------------------------------------------ grid medium
    def set_grid_medium(self, medium):
        """The grid medium of the uploaded scene (include/nori_hip.h, "Grid medium"): a scene.GridMedium, which replaces any medium
        set before, or None to unset a grid medium.  Holds until the next upload."""
        d = medium.desc() if medium is not None else None
        self._check(self._lib.nori_hip_set_grid_medium(self._h, C.byref(d) if d is not None else None), "set_grid_medium")
        return self

    @property
    def grid_medium(self):
        """The record of the grid medium set, as the context stores it, without the voxels: a dict, or None."""
        d = capi.GridMediumDesc()
        rc = self._lib.nori_hip_get_grid_medium(self._h, C.byref(d))
        if rc < 0:
            self._check(rc, "get_grid_medium")
        if rc != 1:
            return None
        return {"shape": (int(d.nz), int(d.ny), int(d.nx)), "bmin": tuple(float(x) for x in d.bmin), "bmax": tuple(float(x) for x in d.bmax),
                "sigma_scale": float(d.sigma_scale), "albedo": tuple(float(x) for x in d.albedo), "g": float(d.g)}

    def _grid_rays(self, o, d, t):
        a, b = _f32(o, 3), _f32(d, 3)
        x = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
        assert a.shape == b.shape and a.shape[0] == x.shape[0]
        return a, b, x

    def grid_medium_distance(self, o, d, tmax, xi):
        """The free flights the (n,) samples xi select on the rays (o, d: (n, 3)) over [0, tmax], as Li draws them; +inf: no event."""
        a, b, t = self._grid_rays(o, d, tmax)
        x = np.ascontiguousarray(xi, dtype=np.float32).reshape(-1)
        assert x.shape[0] == t.shape[0]
        s = np.zeros(t.shape[0], np.float32)
        self._check(self._lib.nori_hip_grid_medium_distance(self._h, ptr(a), ptr(b), ptr(t), ptr(x), t.shape[0], ptr(s)), "grid_medium_distance")
        return s

    def grid_medium_transmittance(self, o, d, dist):
        """Tr = exp(-tau) of the rays (o, d: (n, 3)) over [0, dist]; dist may be infinite."""
        a, b, t = self._grid_rays(o, d, dist)
        tr = np.zeros(t.shape[0], np.float32)
        self._check(self._lib.nori_hip_grid_medium_transmittance(self._h, ptr(a), ptr(b), ptr(t), t.shape[0], ptr(tr)), "grid_medium_transmittance")
        return tr

    def grid_medium_optical_depth(self, o, d, tmax):
        """(tau (n,), voxels visited (n,) int32) of the rays (o, d: (n, 3)) over [0, tmax]."""
        a, b, t = self._grid_rays(o, d, tmax)
        tau, steps = np.zeros(t.shape[0], np.float32), np.zeros(t.shape[0], np.int32)
        self._check(self._lib.nori_hip_grid_medium_optical_depth(self._h, ptr(a), ptr(b), ptr(t), t.shape[0], ptr(tau), ptr(steps)), "grid_medium_optical_depth")
        return tau, steps

    # ------------------------------------------------------------ environment map
    def set_environment(self, env):
        """The environment-map emitter of the uploaded scene (include/nori_hip.h, "Environment-map emitter"): a scene.Environment, or
        None for no environment -- the kernels and the bits of a context that never had one.  Holds until the next upload."""
        if env is None:
            self._check(self._lib.nori_hip_set_environment(self._h, None), "set_environment")
        else:
            d = env.desc()
            self._check(self._lib.nori_hip_set_environment(self._h, C.byref(d)), "set_environment")
        return self

    @property
    def environment_size(self) -> int:
        """N of the environment map set, 0: none."""
        n = C.c_uint32(0)
        self._check(self._lib.nori_hip_get_environment(self._h, C.byref(n)), "get_environment")
        return int(n.value)

    def env_eval(self, dirs, pdf: bool = True):
        """(Le (n, 3), pdf (n,)) of the (n, 3) world directions -- or Le alone with pdf=False -- by the lookup the path uses."""
        d = _f32(dirs, 3)
        rgb = np.zeros((d.shape[0], 3), np.float32)
        p = np.zeros(d.shape[0], np.float32) if pdf else None
        self._check(self._lib.nori_hip_env_eval(self._h, ptr(d), d.shape[0], ptr(rgb), ptr(p)), "env_eval")
        return (rgb, p) if pdf else rgb

    def env_sample(self, xi):
        """(directions (n, 3), Le (n, 3), pdf (n,)) the (n, 2) samples select, as an emitter sample of the path draws them."""
        x = _f32(xi, 2)
        n = x.shape[0]
        d, rgb, p = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        self._check(self._lib.nori_hip_env_sample(self._h, ptr(x), n, ptr(d), ptr(rgb), ptr(p)), "env_sample")
        return d, rgb, p

    def env_tables(self):
        """(row_cdf (N + 1,), col_cdf (N, N + 1), texel_weight (N, N)) as the device built and holds them."""
        n = self.environment_size
        rows, cols, w = np.zeros(n + 1, np.float32), np.zeros((n, n + 1), np.float32), np.zeros((n, n), np.float32)
        self._check(self._lib.nori_hip_debug_env_tables(self._h, ptr(rows), ptr(cols), ptr(w)), "debug_env_tables")
        return rows, cols, w

    def set_lens(self, radius: float, focus_distance: float = 1.0):
        """The thin lens of the uploaded scene's camera (include/nori_hip.h, "Thin-lens camera"): aperture radius and focus distance
        in camera space.  radius 0 is the pinhole, bit for bit.  Holds until the next upload."""
        self._check(self._lib.nori_hip_set_lens(self._h, float(radius), float(focus_distance)), "set_lens")
        return self

    @property
    def lens(self):
        """(radius, focus_distance) as set."""
        r, f = C.c_float(0.0), C.c_float(0.0)
        self._check(self._lib.nori_hip_get_lens(self._h, C.byref(r), C.byref(f)), "get_lens")
        return float(r.value), float(f.value)

    def build_accel(self, builder: int = 0):
        self._check(self._lib.nori_hip_build_accel(self._h, int(builder)), "build_accel")

    def set_option(self, key: str, value) -> None:
        self._check(self._lib.nori_hip_set_option(self._h, key.encode(), str(value).encode()), f"set_option({key})")

    def accel_info(self) -> dict:
        info = capi.AccelInfo()
        self._check(self._lib.nori_hip_accel_info(self._h, C.byref(info)), "accel_info")
        return info.as_dict()

    @property
    def border(self) -> int:
        b = self._lib.nori_hip_border_size(self._h)
        if b < 0:
            self._check(b, "border_size")
        return b

    def frame_shape(self):
        b = self.border
        c = self.scene.camera
        return (c.height + 2 * b, c.width + 2 * b, 4)

    # ---------------------------------------------------- operator-level twins
    def intersect(self, rays: np.ndarray, shadow: bool = False) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=capi.RAY_DTYPE)
        its = np.zeros(rays.shape[0], dtype=capi.ITS_DTYPE)
        self._check(self._lib.nori_hip_intersect(self._h, ptr(rays), ptr(its), rays.shape[0], int(shadow)), "intersect")
        return its

    def texture_eval(self, index: int, uv) -> np.ndarray:
        """(n, 3) float32: Scene.textures[index] (0-based) of the uploaded scene at the (n, 2) texture coordinates uv, evaluated on
        the device by the lookup the shading uses."""
        uv = _f32(uv, 2)
        out = np.zeros((uv.shape[0], 3), dtype=np.float32)
        self._check(self._lib.nori_hip_texture_eval(self._h, int(index) + 1, ptr(uv), uv.shape[0], ptr(out)), "texture_eval")
        return out

    def sample_rays(self, pixel_samples) -> np.ndarray:
        ps = _f32(pixel_samples, 2)
        rays = np.zeros(ps.shape[0], dtype=capi.RAY_DTYPE)
        self._check(self._lib.nori_hip_sample_rays(self._h, ptr(ps), ps.shape[0], ptr(rays)), "sample_rays")
        return rays

    def sample_rays_lens(self, pixel_samples, aperture_samples) -> np.ndarray:
        """The camera ray the render kernels take for (pixelSample, apertureSample) with the context's lens; with radius 0 the
        bits of sample_rays."""
        ps, ap = _f32(pixel_samples, 2), _f32(aperture_samples, 2)
        if ps.shape[0] != ap.shape[0]:
            raise ValueError("sample_rays_lens: one aperture sample per pixel sample")
        rays = np.zeros(ps.shape[0], dtype=capi.RAY_DTYPE)
        self._check(self._lib.nori_hip_sample_rays_lens(self._h, ptr(ps), ptr(ap), ps.shape[0], ptr(rays)), "sample_rays_lens")
        return rays

    def li(self, rays, seed_state, seed_seq) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=capi.RAY_DTYPE)
        ss = np.ascontiguousarray(seed_state, dtype=np.uint64)
        sq = np.ascontiguousarray(seed_seq, dtype=np.uint64)
        out = np.zeros((rays.shape[0], 3), dtype=np.float32)
        self._check(self._lib.nori_hip_li(self._h, ptr(rays), rays.shape[0], ptr(ss), ptr(sq), ptr(out)), "li")
        return out

    def bsdf_sample(self, bsdf: Bsdf, wi, sample):
        wi, sample = _f32(wi, 3), _f32(sample, 2)
        n = wi.shape[0]
        wo, w = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        eta, meas = np.zeros(n, np.float32), np.zeros(n, np.int32)
        d = bsdf.desc()
        self._check(self._lib.nori_hip_bsdf_sample(self._h, C.byref(d), ptr(wi), ptr(sample), n, ptr(wo), ptr(w),
                                                   ptr(eta), ptr(meas)), "bsdf_sample")
        return wo, w, eta, meas

    def bsdf_eval(self, bsdf: Bsdf, wi, wo):
        wi, wo = _f32(wi, 3), _f32(wo, 3)
        out = np.zeros((wi.shape[0], 3), np.float32)
        d = bsdf.desc()
        self._check(self._lib.nori_hip_bsdf_eval(self._h, C.byref(d), ptr(wi), ptr(wo), wi.shape[0], ptr(out)), "bsdf_eval")
        return out

    def bsdf_pdf(self, bsdf: Bsdf, wi, wo):
        wi, wo = _f32(wi, 3), _f32(wo, 3)
        out = np.zeros(wi.shape[0], np.float32)
        d = bsdf.desc()
        self._check(self._lib.nori_hip_bsdf_pdf(self._h, C.byref(d), ptr(wi), ptr(wo), wi.shape[0], ptr(out)), "bsdf_pdf")
        return out

    def warp(self, name: str, sample, param: float = 0.0):
        s = _f32(sample, 2)
        out = np.zeros((s.shape[0], 3), np.float32)
        self._check(self._lib.nori_hip_warp(self._h, capi.WARP_NAMES[name], float(param), ptr(s), s.shape[0], ptr(out)), "warp")
        return out

    def warp_pdf(self, name: str, points, param: float = 0.0):
        p = _f32(points, 3)
        out = np.zeros(p.shape[0], np.float32)
        self._check(self._lib.nori_hip_warp_pdf(self._h, capi.WARP_NAMES[name], float(param), ptr(p), p.shape[0], ptr(out)), "warp_pdf")
        return out

    def arith(self, op_name: str, a, b=None) -> np.ndarray:
        """float32 array of a's shape: the device's own `op_name` (capi.ARITH_OP_NAMES: rcp, div, div_shared, sqrt, slab_rcp, sin,
        cos, log, exp) of every element of a -- and of b for the two quotients -- through the functions the kernels call
        (include/nori_hip.h: nori_hip_debug_arith)."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        binary = op_name in ("div", "div_shared")
        if binary != (b is not None):
            raise ValueError(f"arith({op_name}): takes {'two operands' if binary else 'one operand'}")
        if binary:
            b = np.ascontiguousarray(b, dtype=np.float32)
            if b.shape != a.shape:
                raise ValueError(f"arith({op_name}): operands of shapes {a.shape} and {b.shape}")
        out = np.zeros_like(a)
        self._check(self._lib.nori_hip_debug_arith(self._h, capi.ARITH_OP_NAMES[op_name], ptr(a), ptr(b), a.size, ptr(out)), f"debug_arith({op_name})")
        return out

    def emitter_sample(self, samples, reader="global"):
        """(mesh uint32 [n], tri uint32 [n], p float32 [n, 3]): the emitter's mesh, the triangle within it and the point on it that the
        device's emitter_pick / emitter_point select for each sample (xiE, xiT, xi1, xi2) of `samples` [n, 4], the tables read as
        `reader` says (capi.TABLES_READER_NAMES or its number; include/nori_hip.h: nori_hip_debug_emitter_sample)."""
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1, 4)
        n = x.shape[0]
        mesh, tri, p = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 3), np.float32)
        rd = capi.TABLES_READER_NAMES[reader] if isinstance(reader, str) else int(reader)
        self._check(self._lib.nori_hip_debug_emitter_sample(self._h, rd, ptr(x), n, ptr(mesh), ptr(tri), ptr(p)), f"debug_emitter_sample({reader})")
        return mesh, tri, p

    def emitter_tables(self) -> dict:
        """The scene's emitter tables as they are in device memory (include/nori_hip.h: nori_hip_debug_emitter_tables): n_meshes,
        n_emitters, n_cdf, emitters [n_emitters], cdf_offset / n_triangles / inv_area [n_meshes], cdf [n_cdf]."""
        counts = np.zeros(3, np.uint32)
        self._check(self._lib.nori_hip_debug_emitter_tables(self._h, ptr(counts), None, None, None, None, None), "debug_emitter_tables")
        nm, ne, nc = (int(c) for c in counts)
        em, off, nt = np.zeros(max(ne, 1), np.uint32), np.zeros(max(nm, 1), np.uint32), np.zeros(max(nm, 1), np.uint32)
        inv, cdf = np.zeros(max(nm, 1), np.float32), np.zeros(max(nc, 1), np.float32)
        self._check(self._lib.nori_hip_debug_emitter_tables(self._h, ptr(counts), ptr(em), ptr(off), ptr(nt), ptr(inv), ptr(cdf)), "debug_emitter_tables")
        return {"n_meshes": nm, "n_emitters": ne, "n_cdf": nc, "emitters": em[:ne], "cdf_offset": off[:nm], "n_triangles": nt[:nm],
                "inv_area": inv[:nm], "cdf": cdf[:nc]}

    def tree(self) -> dict:
        """The tree as it is in device memory (include/nori_hip.h: nori_hip_debug_tree): root (the root's link code), n_nodes, n_pairs,
        wide, records_32b, nodes [n_nodes, 16] float32, pairs [n_pairs, 24] float32 and -- None without 32-B records -- nodes32
        [n_nodes, 8] uint32, grid_mn [3], grid_scale [3] float32."""
        return read_tree(lambda *a: self._check(self._lib.nori_hip_debug_tree(self._h, *a), "debug_tree"))

    def first_lists(self, K: int):
        """(count [n_tiles] uint32, pairs [n_tiles, max(K, 1)] uint32): the per-tile candidate lists of the first pass as the device
        builds them for the context's camera at cap K (include/nori_hip.h: nori_hip_debug_first_lists).  count is the number of
        pair records of a tile's list or 0xffffffff (an overflow tile); pairs[tile, :count] index Renderer.tree()["pairs"]."""
        ty, tx = self.tile_grid()
        count, pairs = np.zeros(ty * tx, np.uint32), np.zeros((ty * tx, max(int(K), 1)), np.uint32)
        self._check(self._lib.nori_hip_debug_first_lists(self._h, int(K), ptr(count), ptr(pairs)), "debug_first_lists")
        return count, pairs

    def extend(self, origins, dir_a=None, dir_b=None, maxt_b=None, flags=None, count_traversal=False):
        """wf_extend, the wavefront engine's traversal kernel, on rays of the caller's (include/nori_hip.h: nori_hip_debug_extend).
        Slot k starts at origins[k]; dir_a [n, 3]: its continuation ray (closest hit), dir_b [n, 3] with maxt_b [n] (default inf): its
        shadow ray (any hit).  flags [n] (capi.F_*) default from the directions given: A, B (the path ends on it) or B then A; pass
        them to mix kinds and empty slots (0) in one call -- a direction the flags do not name is not read.
        Returns ((t, u, v, tri, occluded), counts): per slot the closest hit of A (t = inf, tri = capi.EXTEND_MISS_A without one;
        tri is the GLOBAL triangle index) and whether B was occluded; a slot nothing was written to (an empty one) has
        tri = EXTEND_SENTINEL & EXTEND_MISS_A and the sentinel's bits in t, u, v.  counts: closest / shadow queries traced, node /
        triangle tests (with count_traversal)."""
        o = _f32(origins, 3)
        n = o.shape[0]
        if flags is None:
            flags = np.full(n, (capi.F_HAS_A if dir_a is not None else 0) |
                            (0 if dir_b is None else capi.F_HAS_B if dir_a is not None else capi.F_HAS_B | capi.F_END_AFTER_B), np.uint32)
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        da = np.zeros((n, 3), np.float32) if dir_a is None else _f32(dir_a, 3)
        db = np.zeros((n, 4), np.float32)
        db[:, 3] = np.inf
        if dir_b is not None:
            db[:, :3] = _f32(dir_b, 3)
        if maxt_b is not None:
            db[:, 3] = np.asarray(maxt_b, dtype=np.float32)
        if not (da.shape[0] == n and db.shape[0] == n and flags.shape == (n,)):
            raise ValueError("extend: origins, directions and flags of different lengths")
        hits = np.zeros((n, 4), np.float32)
        counts = (C.c_ulonglong * 4)()
        self._check(self._lib.nori_hip_debug_extend(self._h, ptr(o), ptr(da), ptr(db), ptr(flags), n, int(bool(count_traversal)), ptr(hits), counts), "debug_extend")
        word = hits[:, 3].copy().view(np.uint32)
        names = ("n_closest_rays", "n_shadow_rays", "n_node_tests", "n_tri_tests")
        return ((hits[:, 0].copy(), hits[:, 1].copy(), hits[:, 2].copy(), word & np.uint32(capi.EXTEND_MISS_A), (word >> 31).astype(bool)),
                {k: int(v) for k, v in zip(names, counts)})

    def pcg32_floats(self, seed_state, seed_seq, count: int):
        ss = np.ascontiguousarray(seed_state, dtype=np.uint64)
        sq = np.ascontiguousarray(seed_seq, dtype=np.uint64)
        out = np.zeros((ss.shape[0], count), np.float32)
        self._check(self._lib.nori_hip_pcg32_floats(self._h, ptr(ss), ptr(sq), ss.shape[0], count, ptr(out)), "pcg32_floats")
        return out

    def splat(self, positions, values, rgbw: Optional[np.ndarray] = None):
        p, v = _f32(positions, 2), _f32(values, 3)
        if rgbw is None:
            rgbw = np.zeros(self.frame_shape(), np.float32)
        rgbw = np.ascontiguousarray(rgbw, dtype=np.float32)
        self._check(self._lib.nori_hip_splat(self._h, ptr(p), ptr(v), p.shape[0], ptr(rgbw)), "splat")
        return rgbw

    # ------------------------------------------------------------ hot path
    @staticmethod
    def _params(spp_begin, spp_count, tile_mod, tile_rem, count_traversal, stream, time_kernels=False, seed_mode=capi.SEED_PER_SAMPLE):
        p = capi.RenderParams()
        p.spp_begin, p.spp_count = int(spp_begin), int(spp_count)
        p.tile_mod, p.tile_rem = int(tile_mod), int(tile_rem)
        p.seed_mode = int(seed_mode)
        p.count_traversal = int(bool(count_traversal))
        p.time_kernels = int(bool(time_kernels))
        p.stream = stream
        return p

    def render_host(self, spp_count=None, spp_begin=0, tile_mod=1, tile_rem=0, count_traversal=False, seed_mode=capi.SEED_PER_SAMPLE):
        """Render into a fresh host RGBW frame; returns (rgbw, stats dict).  seed_mode: capi.SEED_PER_SAMPLE (default)
        or capi.SEED_NORI_BLOCK -- the reference's one-stream-per-32x32-block sampler (src/independent.cpp:36-41)."""
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, tile_mod, tile_rem, count_traversal, None, seed_mode=seed_mode)
        rgbw = np.zeros(self.frame_shape(), np.float32)
        st = capi.RenderStats()
        self._check(self._lib.nori_hip_render_host(self._h, C.byref(p), ptr(rgbw), C.byref(st)), "render_host")
        return rgbw, st.as_dict()

    def render_into(self, rgbw_tensor, spp_count=None, spp_begin=0, tile_mod=1, tile_rem=0,
                    count_traversal=False, stream=None, want_stats=True, time_kernels=False):
        """Accumulate into a torch CUDA float32 tensor of shape frame_shape().

        `stream`: a torch.cuda.Stream (its raw hipStream_t is handed to the
        library) or None for the legacy default stream."""
        assert rgbw_tensor.is_cuda and rgbw_tensor.is_contiguous() and tuple(rgbw_tensor.shape) == tuple(self.frame_shape())
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, tile_mod, tile_rem, count_traversal, raw, time_kernels)
        st = capi.RenderStats() if want_stats else None
        self._check(self._lib.nori_hip_render(self._h, C.byref(p), C.c_void_p(rgbw_tensor.data_ptr()),
                                              C.byref(st) if st is not None else None), "render")
        return st.as_dict() if st is not None else None

    # -- second moments, error map, render to a target error (include/nori_hip.h) --
    def _is_frame(self, t):
        return t.is_cuda and t.is_contiguous() and tuple(t.shape) == tuple(self.frame_shape()) and str(t.dtype) == "torch.float32"

    def render_moments_into(self, rgbw_tensor, m2_tensor, spp_count=None, spp_begin=0, tile_mod=1, tile_rem=0,
                            count_traversal=False, stream=None, want_stats=True, time_kernels=False, seed_mode=capi.SEED_PER_SAMPLE):
        """render_into, and the same samples' second moments accumulated into `m2_tensor` (shape and layout of the frame):
        per tap of weight w the frame receives (L w, w), the moment frame (float32(L L) w, float32(w w))."""
        assert self._is_frame(rgbw_tensor) and self._is_frame(m2_tensor)
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, tile_mod, tile_rem, count_traversal, raw, time_kernels, seed_mode)
        st = capi.RenderStats() if want_stats else None
        self._check(self._lib.nori_hip_render_moments(self._h, C.byref(p), C.c_void_p(rgbw_tensor.data_ptr()), C.c_void_p(m2_tensor.data_ptr()),
                                                      C.byref(st) if st is not None else None), "render_moments")
        return st.as_dict() if st is not None else None

    def render_moments_host(self, spp_count=None, spp_begin=0, tile_mod=1, tile_rem=0, count_traversal=False, seed_mode=capi.SEED_PER_SAMPLE):
        """Render into fresh host frames; returns (rgbw, m2, stats dict)."""
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, tile_mod, tile_rem, count_traversal, None, seed_mode=seed_mode)
        rgbw, m2 = np.zeros(self.frame_shape(), np.float32), np.zeros(self.frame_shape(), np.float32)
        st = capi.RenderStats()
        self._check(self._lib.nori_hip_render_moments_host(self._h, C.byref(p), ptr(rgbw), ptr(m2), C.byref(st)), "render_moments_host")
        return rgbw, m2, st.as_dict()

    def error_map(self, rgbw, m2, threshold=0.0, stream=None):
        """(err, summary dict): the per-pixel relative standard error of the mean (height x width, no border) of a frame and its
        moment frame, and its deterministic summary (sum_err, max_err, threshold, n_pixels, n_empty, n_above).  Torch CUDA
        tensors give a CUDA tensor; numpy arrays are copied to the device and give a numpy array."""
        c = self.scene.camera
        out = capi.ErrorSummary()
        if isinstance(rgbw, np.ndarray):
            rgbw, m2 = (np.ascontiguousarray(a, dtype=np.float32) for a in (rgbw, m2))
            assert rgbw.shape == m2.shape == tuple(self.frame_shape())
            err = np.zeros((c.height, c.width), np.float32)
            self._check(self._lib.nori_hip_error_map_host(self._h, ptr(rgbw), ptr(m2), ptr(err), float(threshold), C.byref(out)), "error_map_host")
            return err, out.as_dict()
        import torch
        assert self._is_frame(rgbw) and self._is_frame(m2)
        err = torch.empty((c.height, c.width), dtype=torch.float32, device=rgbw.device)
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._lib.nori_hip_error_map(self._h, C.c_void_p(rgbw.data_ptr()), C.c_void_p(m2.data_ptr()), C.c_void_p(err.data_ptr()),
                                                 float(threshold), C.byref(out), raw), "error_map")
        return err, out.as_dict()

    def render_to_error(self, rgbw_tensor, m2_tensor, target_mean_err, pass_spp=16, spp_count=None, spp_begin=0, stream=None,
                        count_traversal=False, time_kernels=False):
        """Render in passes of `pass_spp` samples per pixel, at most `spp_count` (default: the scene's sample count), until the
        mean of the error map is at most `target_mean_err`; accumulates into both tensors.  Returns (spp_done, summary dict,
        stats dict with counters and times summed over the passes)."""
        assert self._is_frame(rgbw_tensor) and self._is_frame(m2_tensor)
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, 1, 0, count_traversal, raw, time_kernels)
        done, last, st = C.c_uint32(0), capi.ErrorSummary(), capi.RenderStats()
        self._check(self._lib.nori_hip_render_to_error(self._h, C.byref(p), int(pass_spp), float(target_mean_err), C.c_void_p(rgbw_tensor.data_ptr()),
                                                       C.c_void_p(m2_tensor.data_ptr()), C.byref(done), C.byref(last), C.byref(st)), "render_to_error")
        return int(done.value), last.as_dict(), st.as_dict()

    # -- tile lists, tile errors, selection, adaptive sampling (include/nori_hip.h) --
    def tile_grid(self):
        """(tiles_y, tiles_x) of the frame's 16x16 tiles; tile t = ty * tiles_x + tx"""
        c = self.scene.camera
        return ((c.height + capi.TILE_SIZE - 1) // capi.TILE_SIZE, (c.width + capi.TILE_SIZE - 1) // capi.TILE_SIZE)

    @staticmethod
    def _tile_list(tiles):
        return np.ascontiguousarray(np.asarray(list(tiles) if not isinstance(tiles, np.ndarray) else tiles).reshape(-1), dtype=np.uint32)

    def render_tiles_into(self, tiles, rgbw_tensor, m2_tensor=None, spp_count=None, spp_begin=0, count_traversal=False, stream=None,
                          want_stats=True, time_kernels=False, seed_mode=capi.SEED_PER_SAMPLE):
        """render_moments_into (render_into where m2_tensor is None) for exactly the listed tiles: strictly ascending raster ids."""
        assert self._is_frame(rgbw_tensor) and (m2_tensor is None or self._is_frame(m2_tensor))
        t = self._tile_list(tiles)
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, 1, 0, count_traversal, raw, time_kernels, seed_mode)
        st = capi.RenderStats() if want_stats else None
        self._check(self._lib.nori_hip_render_tiles(self._h, C.byref(p), ptr(t), t.shape[0], C.c_void_p(rgbw_tensor.data_ptr()),
                                                    C.c_void_p(m2_tensor.data_ptr()) if m2_tensor is not None else None,
                                                    C.byref(st) if st is not None else None), "render_tiles")
        return st.as_dict() if st is not None else None

    def render_tiles_host(self, tiles, spp_count=None, spp_begin=0, count_traversal=False, seed_mode=capi.SEED_PER_SAMPLE):
        """The listed tiles into fresh host frames; returns (rgbw, m2, stats dict)."""
        t = self._tile_list(tiles)
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, 1, 0, count_traversal, None, seed_mode=seed_mode)
        rgbw, m2 = np.zeros(self.frame_shape(), np.float32), np.zeros(self.frame_shape(), np.float32)
        st = capi.RenderStats()
        self._check(self._lib.nori_hip_render_tiles_host(self._h, C.byref(p), ptr(t), t.shape[0], ptr(rgbw), ptr(m2), C.byref(st)), "render_tiles_host")
        return rgbw, m2, st.as_dict()

    def tile_errors(self, rgbw, m2, stream=None):
        """(tiles_y, tiles_x) float32: the mean of the error map over each tile's pixels inside the frame.  Torch CUDA tensors give a
        CUDA tensor; numpy arrays are copied to the device and give a numpy array."""
        if isinstance(rgbw, np.ndarray):
            rgbw, m2 = (np.ascontiguousarray(a, dtype=np.float32) for a in (rgbw, m2))
            assert rgbw.shape == m2.shape == tuple(self.frame_shape())
            out = np.zeros(self.tile_grid(), np.float32)
            self._check(self._lib.nori_hip_tile_errors_host(self._h, ptr(rgbw), ptr(m2), ptr(out)), "tile_errors_host")
            return out
        import torch
        assert self._is_frame(rgbw) and self._is_frame(m2)
        out = torch.empty(self.tile_grid(), dtype=torch.float32, device=rgbw.device)
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._lib.nori_hip_tile_errors(self._h, C.c_void_p(rgbw.data_ptr()), C.c_void_p(m2.data_ptr()), C.c_void_p(out.data_ptr()), raw), "tile_errors")
        return out

    def select_tiles(self, tile_err, target, tiles):
        """uint32 array: the tiles of `tiles` (strictly ascending) with not (tile_err[t] <= target), in order -- a NaN stays in.
        tile_err: one float per tile of the frame, a torch CUDA tensor or a numpy array (copied to the device)."""
        import torch
        if isinstance(tile_err, np.ndarray):
            tile_err = torch.from_numpy(np.ascontiguousarray(tile_err, dtype=np.float32)).to(f"cuda:{self.device}")
        ty, tx = self.tile_grid()
        assert tile_err.is_cuda and tile_err.is_contiguous() and tile_err.numel() == ty * tx and str(tile_err.dtype) == "torch.float32"
        t = self._tile_list(tiles)
        out, n = np.zeros(max(t.shape[0], 1), np.uint32), C.c_uint32(0)
        torch.cuda.synchronize(tile_err.device)      # the call runs on the default stream
        self._check(self._lib.nori_hip_select_tiles(self._h, C.c_void_p(tile_err.data_ptr()), float(target), ptr(t), t.shape[0], ptr(out), C.byref(n)), "select_tiles")
        return out[:int(n.value)].copy()

    def render_adaptive(self, rgbw_tensor, m2_tensor, target_tile_err, pass_spp=16, spp_count=None, spp_begin=0, stream=None,
                        count_traversal=False, time_kernels=False):
        """render_to_error with the samples steered by the tile errors: passes of `pass_spp` samples per pixel over the tiles whose
        error is still above `target_tile_err`, at most `spp_count` per pixel; accumulates into both tensors.  Returns (tile_spp: a
        (tiles_y, tiles_x) int32 CUDA tensor of the samples each tile received, summary dict, stats dict)."""
        import torch
        assert self._is_frame(rgbw_tensor) and self._is_frame(m2_tensor)
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, 1, 0, count_traversal, raw, time_kernels)
        tile_spp = torch.zeros(self.tile_grid(), dtype=torch.int32, device=rgbw_tensor.device)
        out, st = capi.AdaptiveSummary(), capi.RenderStats()
        self._check(self._lib.nori_hip_render_adaptive(self._h, C.byref(p), int(pass_spp), float(target_tile_err), C.c_void_p(rgbw_tensor.data_ptr()),
                                                       C.c_void_p(m2_tensor.data_ptr()), C.c_void_p(tile_spp.data_ptr()), C.byref(out), C.byref(st)), "render_adaptive")
        return tile_spp, out.as_dict(), st.as_dict()

    def render_adaptive_host(self, target_tile_err, pass_spp=16, spp_count=None, spp_begin=0, count_traversal=False):
        """The adaptive loop into fresh host frames; returns (rgbw, m2, err, tile_spp, summary dict, stats dict)."""
        c = self.scene.camera
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, 1, 0, count_traversal, None)
        rgbw, m2 = np.zeros(self.frame_shape(), np.float32), np.zeros(self.frame_shape(), np.float32)
        err, tile_spp = np.zeros((c.height, c.width), np.float32), np.zeros(self.tile_grid(), np.uint32)
        out, st = capi.AdaptiveSummary(), capi.RenderStats()
        self._check(self._lib.nori_hip_render_adaptive_host(self._h, C.byref(p), int(pass_spp), float(target_tile_err), ptr(rgbw), ptr(m2), ptr(err),
                                                            ptr(tile_spp), C.byref(out), C.byref(st)), "render_adaptive_host")
        return rgbw, m2, err, tile_spp, out.as_dict(), st.as_dict()

    # -- first-hit feature frames: albedo, shading normal, depth (include/nori_hip.h: nori_hip_render_features) --
    def render_features_into(self, albedo=None, normal=None, depth=None, spp_count=None, spp_begin=0, tile_mod=1, tile_rem=0, stream=None,
                             time_kernels=False, want_stats=True, seed_mode=capi.SEED_PER_SAMPLE, features=None):
        """Accumulate the first-hit feature frames into the torch CUDA frame tensors given (shape and layout of render_into's): one
        closest-hit ray per camera sample, the camera samples of render_into.  The mask follows from which tensors are given
        (`features`, a nori_feature mask, overrides it: for the error paths).  Decode with develop_features_host."""
        given = {"albedo": albedo, "normal": normal, "depth": depth}
        mask = 0
        for name, t in given.items():
            if t is not None:
                assert self._is_frame(t), name
                mask |= capi.FEATURE_BITS[name]
        if features is not None:
            mask = int(features)
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, tile_mod, tile_rem, False, raw, time_kernels, seed_mode)
        st = capi.RenderStats() if want_stats else None
        d = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (albedo, normal, depth)]
        self._check(self._lib.nori_hip_render_features(self._h, C.byref(p), mask, d[0], d[1], d[2], C.byref(st) if st is not None else None), "render_features")
        return st.as_dict() if st is not None else None

    def render_features_host(self, features=("albedo", "normal", "depth"), spp_count=None, spp_begin=0, tile_mod=1, tile_rem=0,
                             time_kernels=False, seed_mode=capi.SEED_PER_SAMPLE):
        """The named feature frames into fresh host frames; returns (dict name -> RGBW frame, stats dict)."""
        names = [features] if isinstance(features, str) else list(features)
        mask = 0
        for name in names:
            mask |= capi.FEATURE_BITS[name]
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, tile_mod, tile_rem, False, None, time_kernels, seed_mode)
        frames = {name: np.zeros(self.frame_shape(), np.float32) for name in ("albedo", "normal", "depth") if name in names}
        st = capi.RenderStats()
        d = [ptr(frames[name]) if name in frames else None for name in ("albedo", "normal", "depth")]
        self._check(self._lib.nori_hip_render_features_host(self._h, C.byref(p), mask, d[0], d[1], d[2], C.byref(st)), "render_features_host")
        return frames, st.as_dict()

    # -- the denoiser: guide records, NL-means filter (include/nori_hip.h: nori_hip_denoise) --
    def _host_frames(self, rgbw, m2, albedo, normal, depth):
        frames = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (rgbw, m2, albedo, normal, depth)]
        assert frames[0] is not None and frames[1] is not None, "the RGBW frame and the moment frame are required"
        for a in frames:
            assert a is None or a.shape == tuple(self.frame_shape())
        return frames

    def denoise_guides_host(self, rgbw, m2, albedo=None, normal=None, depth=None):
        """Step A for host frames: (height, width, 16) float32 -- mu[3], var[3], albedo[3], normal[3], z, cov, valid, 0 per pixel."""
        frames = self._host_frames(rgbw, m2, albedo, normal, depth)
        c = self.scene.camera
        guides = np.zeros((c.height, c.width, capi.GUIDE_FLOATS), np.float32)
        self._check(self._lib.nori_hip_denoise_guides_host(self._h, *[ptr(a) for a in frames], ptr(guides)), "denoise_guides_host")
        return guides

    def denoise_host(self, rgbw, m2, albedo=None, normal=None, depth=None, **params):
        """Steps A and B for host frames: (rgb (height, width, 3), wsum (height, width)).  params: the fields of nori_denoise_params
        (radius, patch, k_c, alpha, tau_albedo, tau_normal, k_depth, tau_cov), each defaulting to the header's default."""
        frames = self._host_frames(rgbw, m2, albedo, normal, depth)
        c = self.scene.camera
        rgb, wsum = np.zeros((c.height, c.width, 3), np.float32), np.zeros((c.height, c.width), np.float32)
        p = capi.DenoiseParams(**params)
        self._check(self._lib.nori_hip_denoise_host(self._h, C.byref(p), *[ptr(a) for a in frames], ptr(rgb), ptr(wsum)), "denoise_host")
        return rgb, wsum

    def denoise_into(self, rgb_out, rgbw, m2, albedo=None, normal=None, depth=None, wsum=None, stream=None, **params):
        """Steps A and B on torch CUDA tensors: the frames have frame_shape(), rgb_out is (height, width, 3) and wsum, if given,
        (height, width), all float32 and contiguous.  Asynchronous on `stream` (a torch.cuda.Stream, or None for the default one)."""
        c = self.scene.camera
        assert self._is_frame(rgbw) and self._is_frame(m2)
        for t in (albedo, normal, depth):
            assert t is None or self._is_frame(t)
        for t, shape in ((rgb_out, (c.height, c.width, 3)), (wsum, (c.height, c.width))):
            assert t is None or (t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape and str(t.dtype) == "torch.float32")
        p = capi.DenoiseParams(**params)
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        d = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (rgbw, m2, albedo, normal, depth, rgb_out, wsum)]
        self._check(self._lib.nori_hip_denoise(self._h, C.byref(p), *d, raw), "denoise")

    def denoise_guides_into(self, guides, rgbw, m2, albedo=None, normal=None, depth=None, stream=None):
        """Step A on torch CUDA tensors: guides is (height, width, 16) float32."""
        c = self.scene.camera
        assert self._is_frame(rgbw) and self._is_frame(m2)
        assert guides.is_cuda and guides.is_contiguous() and tuple(guides.shape) == (c.height, c.width, capi.GUIDE_FLOATS) and str(guides.dtype) == "torch.float32"
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        d = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (rgbw, m2, albedo, normal, depth, guides)]
        self._check(self._lib.nori_hip_denoise_guides(self._h, *d, raw), "denoise_guides")

    # -- the denoiser with its output variance, the error of a denoised frame, the loop that stops on it (nori_hip_denoise_var) --
    def _pixel_shapes(self):
        c = self.scene.camera
        return (c.height, c.width, 3), (c.height, c.width)

    def _is_pixels(self, t, shape):
        return t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape and str(t.dtype) == "torch.float32"

    def denoise_var_into(self, rgb_out, var_out, rgbw, m2, albedo=None, normal=None, depth=None, wsum=None, tiles=None, stream=None, **params):
        """denoise_into with the variance of the output under fixed weights into var_out (height, width, 3).  tiles: strictly
        ascending raster ids -- only those tiles' pixels are written (the call then synchronises `stream` once) -- or None: the
        whole frame."""
        rgb_shape, px_shape = self._pixel_shapes()
        assert self._is_frame(rgbw) and self._is_frame(m2)
        for t in (albedo, normal, depth):
            assert t is None or self._is_frame(t)
        assert self._is_pixels(rgb_out, rgb_shape) and self._is_pixels(var_out, rgb_shape) and (wsum is None or self._is_pixels(wsum, px_shape))
        p = capi.DenoiseParams(**params)
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        d = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (rgbw, m2, albedo, normal, depth)]
        o = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (rgb_out, var_out, wsum)]
        tl = None if tiles is None else self._tile_list(tiles)
        self._check(self._lib.nori_hip_denoise_var(self._h, C.byref(p), *d, ptr(tl) if tl is not None else None, 0 if tl is None else tl.shape[0], *o, raw), "denoise_var")

    def denoise_var_host(self, rgbw, m2, albedo=None, normal=None, depth=None, tiles=None, out=None, **params):
        """Host frames: (rgb, var (height, width, 3), wsum (height, width)).  With `tiles` only the listed tiles' pixels of `out`
        -- a triple of arrays to write into, fresh zeros by default -- are written."""
        frames = self._host_frames(rgbw, m2, albedo, normal, depth)
        rgb_shape, px_shape = self._pixel_shapes()
        rgb, var, wsum = out if out is not None else (np.zeros(rgb_shape, np.float32), np.zeros(rgb_shape, np.float32), np.zeros(px_shape, np.float32))
        assert rgb.shape == var.shape == rgb_shape and wsum.shape == px_shape and all(a.dtype == np.float32 for a in (rgb, var, wsum))
        p = capi.DenoiseParams(**params)
        tl = None if tiles is None else self._tile_list(tiles)
        self._check(self._lib.nori_hip_denoise_var_host(self._h, C.byref(p), *[ptr(a) for a in frames], ptr(tl) if tl is not None else None,
                                                        0 if tl is None else tl.shape[0], ptr(rgb), ptr(var), ptr(wsum)), "denoise_var_host")
        return rgb, var, wsum

    def denoised_error_map(self, rgb, var, wsum, threshold=0.0, want_map=True, stream=None):
        """error_map for a denoised frame, its variance and its weight sums (as denoise_var writes them): (err (height, width),
        summary dict).  Torch CUDA tensors give a CUDA map; numpy arrays are copied to the device and give a numpy map."""
        rgb_shape, px_shape = self._pixel_shapes()
        s = capi.ErrorSummary()
        if isinstance(rgb, np.ndarray):
            rgb, var, wsum = (np.ascontiguousarray(a, dtype=np.float32) for a in (rgb, var, wsum))
            assert rgb.shape == var.shape == rgb_shape and wsum.shape == px_shape
            err = np.zeros(px_shape, np.float32) if want_map else None
            self._check(self._lib.nori_hip_denoised_error_map_host(self._h, ptr(rgb), ptr(var), ptr(wsum), ptr(err), float(threshold), C.byref(s)), "denoised_error_map_host")
            return err, s.as_dict()
        import torch
        assert self._is_pixels(rgb, rgb_shape) and self._is_pixels(var, rgb_shape) and self._is_pixels(wsum, px_shape)
        err = torch.empty(px_shape, dtype=torch.float32, device=rgb.device) if want_map else None
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._lib.nori_hip_denoised_error_map(self._h, C.c_void_p(rgb.data_ptr()), C.c_void_p(var.data_ptr()), C.c_void_p(wsum.data_ptr()),
                                                          C.c_void_p(err.data_ptr()) if err is not None else None, float(threshold), C.byref(s), raw), "denoised_error_map")
        return err, s.as_dict()

    def denoised_tile_errors(self, rgb, var, wsum, stream=None):
        """tile_errors for a denoised frame: (tiles_y, tiles_x) float32, a CUDA tensor for CUDA tensors, a numpy array for numpy arrays."""
        rgb_shape, px_shape = self._pixel_shapes()
        if isinstance(rgb, np.ndarray):
            rgb, var, wsum = (np.ascontiguousarray(a, dtype=np.float32) for a in (rgb, var, wsum))
            assert rgb.shape == var.shape == rgb_shape and wsum.shape == px_shape
            out = np.zeros(self.tile_grid(), np.float32)
            self._check(self._lib.nori_hip_denoised_tile_errors_host(self._h, ptr(rgb), ptr(var), ptr(wsum), ptr(out)), "denoised_tile_errors_host")
            return out
        import torch
        assert self._is_pixels(rgb, rgb_shape) and self._is_pixels(var, rgb_shape) and self._is_pixels(wsum, px_shape)
        out = torch.empty(self.tile_grid(), dtype=torch.float32, device=rgb.device)
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._lib.nori_hip_denoised_tile_errors(self._h, C.c_void_p(rgb.data_ptr()), C.c_void_p(var.data_ptr()), C.c_void_p(wsum.data_ptr()),
                                                            C.c_void_p(out.data_ptr()), raw), "denoised_tile_errors")
        return out

    def render_adaptive_denoised(self, rgbw_tensor, m2_tensor, target_tile_err, albedo=None, normal=None, depth=None, pass_spp=16, spp_count=None,
                                 spp_begin=0, stream=None, count_traversal=False, time_kernels=False, seed_mode=capi.SEED_PER_SAMPLE, tile_mod=1, **params):
        """render_adaptive with the tiles retired on the error of the DENOISED frame: accumulates into both frame tensors; albedo,
        normal, depth are feature frames rendered beforehand (render_features_into), each optional; params: nori_denoise_params.
        Returns (rgb_out, var_out (height, width, 3), wsum (height, width), tile_spp (tiles_y, tiles_x) int32 -- CUDA tensors --,
        summary dict, stats dict); the first three are denoise_var of the frames as they are left."""
        import torch
        assert self._is_frame(rgbw_tensor) and self._is_frame(m2_tensor)
        for t in (albedo, normal, depth):
            assert t is None or self._is_frame(t)
        rgb_shape, px_shape = self._pixel_shapes()
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, tile_mod, 0, count_traversal, raw, time_kernels, seed_mode)
        dp = capi.DenoiseParams(**params)
        dev = rgbw_tensor.device
        rgb, var = torch.empty(rgb_shape, dtype=torch.float32, device=dev), torch.empty(rgb_shape, dtype=torch.float32, device=dev)
        wsum, tile_spp = torch.empty(px_shape, dtype=torch.float32, device=dev), torch.zeros(self.tile_grid(), dtype=torch.int32, device=dev)
        out, st = capi.AdaptiveSummary(), capi.RenderStats()
        d = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (rgbw_tensor, m2_tensor, albedo, normal, depth, rgb, var, wsum, tile_spp)]
        self._check(self._lib.nori_hip_render_adaptive_denoised(self._h, C.byref(p), int(pass_spp), float(target_tile_err), C.byref(dp), *d, C.byref(out), C.byref(st)),
                    "render_adaptive_denoised")
        return rgb, var, wsum, tile_spp, out.as_dict(), st.as_dict()

    def render_adaptive_denoised_host(self, target_tile_err, albedo=None, normal=None, depth=None, pass_spp=16, spp_count=None, spp_begin=0,
                                      count_traversal=False, **params):
        """The same loop into fresh host arrays; returns a dict: rgbw, m2, rgb, var, wsum, err (the denoised error map), tile_spp,
        summary, stats."""
        feats = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (albedo, normal, depth)]
        for a in feats:
            assert a is None or a.shape == tuple(self.frame_shape())
        rgb_shape, px_shape = self._pixel_shapes()
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, 1, 0, count_traversal, None)
        dp = capi.DenoiseParams(**params)
        r = dict(rgbw=np.zeros(self.frame_shape(), np.float32), m2=np.zeros(self.frame_shape(), np.float32), rgb=np.zeros(rgb_shape, np.float32),
                 var=np.zeros(rgb_shape, np.float32), wsum=np.zeros(px_shape, np.float32), err=np.zeros(px_shape, np.float32),
                 tile_spp=np.zeros(self.tile_grid(), np.uint32))
        out, st = capi.AdaptiveSummary(), capi.RenderStats()
        self._check(self._lib.nori_hip_render_adaptive_denoised_host(self._h, C.byref(p), int(pass_spp), float(target_tile_err), C.byref(dp), ptr(r["rgbw"]), ptr(r["m2"]),
                                                                     *[ptr(a) for a in feats], ptr(r["rgb"]), ptr(r["var"]), ptr(r["wsum"]), ptr(r["err"]),
                                                                     ptr(r["tile_spp"]), C.byref(out), C.byref(st)), "render_adaptive_denoised_host")
        r["summary"], r["stats"] = out.as_dict(), st.as_dict()
        return r

    # -- sample levels per tile from a pilot (include/nori_hip.h: nori_hip_allocate_tiles, nori_hip_render_allocated) --
    @staticmethod
    def allocate_levels(pilot_spp, spp_count):
        """[spp_0 .. spp_J]: spp_j = pilot_spp << j, J = min(7, floor(log2(spp_count / pilot_spp)))"""
        assert pilot_spp >= 1 and spp_count >= pilot_spp
        J = 0
        while J < capi.ALLOC_MAX_LEVEL and (pilot_spp << (J + 1)) <= spp_count:
            J += 1
        return [pilot_spp << j for j in range(J + 1)]

    def allocate_tiles(self, tile_err, target, level, done, pilot_spp=16, spp_count=None, headroom=1.0, max_rounds=1, metric=0):
        """One round of the allocation without a render: (level, done, tiles, bucket_begin) -- the new levels and done flags (uint32,
        one per tile), the moving tiles grouped by pair (i, j) ascending in i then j (ascending id inside a pair), and the 29 offsets of
        the pairs in that array.  tile_err: one float per tile, a torch CUDA tensor or a numpy array (copied to the device)."""
        import torch
        if isinstance(tile_err, np.ndarray):
            tile_err = torch.from_numpy(np.ascontiguousarray(tile_err, dtype=np.float32)).to(f"cuda:{self.device}")
        ty, tx = self.tile_grid()
        assert tile_err.is_cuda and tile_err.is_contiguous() and tile_err.numel() == ty * tx and str(tile_err.dtype) == "torch.float32"
        level = np.array(level, dtype=np.uint32).reshape(-1)
        done = np.array(done, dtype=np.uint32).reshape(-1)
        assert level.size == done.size == ty * tx
        spp = self.scene.sample_count if spp_count is None else spp_count
        ap = capi.AllocateParams(int(pilot_spp), int(max_rounds), float(target), float(headroom), int(metric))
        tiles, begin = np.zeros(ty * tx, np.uint32), np.zeros(capi.ALLOC_MAX_BUCKETS + 1, np.uint32)
        torch.cuda.synchronize(tile_err.device)      # the call runs on the default stream
        self._check(self._lib.nori_hip_allocate_tiles(self._h, C.byref(ap), int(spp), C.c_void_p(tile_err.data_ptr()), ptr(level), ptr(done), ptr(tiles), ptr(begin)),
                    "allocate_tiles")
        return level, done, tiles[:int(begin[-1])].copy(), begin

    def render_allocated(self, rgbw_tensor, m2_tensor, target_tile_err, albedo=None, normal=None, depth=None, metric=0, pilot_spp=16, max_rounds=3, headroom=1.0,
                         spp_count=None, spp_begin=0, stream=None, count_traversal=False, time_kernels=False, **params):
        """The loop of render_allocated_host on torch CUDA tensors: accumulates into both frame tensors.  metric 0 returns (tile_spp
        (tiles_y, tiles_x) int32, level_log (max_rounds + 1, tiles) int32, summary dict, stats dict); metric 1 (the denoised error; the
        feature frames and the nori_denoise_params count) returns (rgb_out, var_out, wsum, tile_spp, level_log, summary dict, stats dict)."""
        import torch
        assert self._is_frame(rgbw_tensor) and self._is_frame(m2_tensor)
        for t in (albedo, normal, depth):
            assert t is None or self._is_frame(t)
        rgb_shape, px_shape = self._pixel_shapes()
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, 1, 0, count_traversal, raw, time_kernels)
        ap = capi.AllocateParams(int(pilot_spp), int(max_rounds), float(target_tile_err), float(headroom), int(metric))
        dp = capi.DenoiseParams(**params)
        dev = rgbw_tensor.device
        ty, tx = self.tile_grid()
        tile_spp = torch.zeros((ty, tx), dtype=torch.int32, device=dev)
        level_log = torch.zeros((int(max_rounds) + 1, ty * tx), dtype=torch.int32, device=dev)
        outs = [None, None, None]
        if metric == 1:
            outs = [torch.empty(rgb_shape, dtype=torch.float32, device=dev), torch.empty(rgb_shape, dtype=torch.float32, device=dev),
                    torch.empty(px_shape, dtype=torch.float32, device=dev)]
        out, st = capi.AdaptiveSummary(), capi.RenderStats()
        d = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (rgbw_tensor, m2_tensor, albedo, normal, depth, *outs, tile_spp, level_log)]
        self._check(self._lib.nori_hip_render_allocated(self._h, C.byref(p), C.byref(ap), C.byref(dp), *d, C.byref(out), C.byref(st)), "render_allocated")
        tail = (tile_spp, level_log, out.as_dict(), st.as_dict())
        return tail if metric != 1 else (*outs, *tail)

    def _render_allocated_host(self, metric, target_tile_err, feats, pilot_spp, max_rounds, headroom, spp_count, spp_begin, count_traversal, seed_mode, tile_mod, params):
        feats = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in feats]
        for a in feats:
            assert a is None or a.shape == tuple(self.frame_shape())
        rgb_shape, px_shape = self._pixel_shapes()
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = self._params(spp_begin, spp, tile_mod, 0, count_traversal, None, seed_mode=seed_mode)
        ap = capi.AllocateParams(int(pilot_spp), int(max_rounds), float(target_tile_err), float(headroom), int(metric))
        dp = capi.DenoiseParams(**params)
        n_tiles = self.tile_grid()[0] * self.tile_grid()[1]
        r = dict(rgbw=np.zeros(self.frame_shape(), np.float32), m2=np.zeros(self.frame_shape(), np.float32), err=np.zeros(px_shape, np.float32),
                 tile_spp=np.zeros(self.tile_grid(), np.uint32), level_log=np.zeros((max(int(max_rounds), 0) + 1, n_tiles), np.uint32))
        if metric == 1:
            r.update(rgb=np.zeros(rgb_shape, np.float32), var=np.zeros(rgb_shape, np.float32), wsum=np.zeros(px_shape, np.float32))
        out, st = capi.AdaptiveSummary(), capi.RenderStats()
        self._check(self._lib.nori_hip_render_allocated_host(self._h, C.byref(p), C.byref(ap), C.byref(dp), ptr(r["rgbw"]), ptr(r["m2"]), *[ptr(a) for a in feats],
                                                             ptr(r.get("rgb")), ptr(r.get("var")), ptr(r.get("wsum")), ptr(r["err"]), ptr(r["tile_spp"]),
                                                             ptr(r["level_log"]), C.byref(out), C.byref(st)), "render_allocated_host")
        r["summary"], r["stats"] = out.as_dict(), st.as_dict()
        return r

    def render_allocated_host(self, target_tile_err, pilot_spp=16, max_rounds=3, headroom=1.0, spp_count=None, spp_begin=0, count_traversal=False,
                              seed_mode=capi.SEED_PER_SAMPLE, tile_mod=1):
        """Render to a tile error in few passes: a pilot of `pilot_spp` samples per pixel, then at most `max_rounds` rounds that move
        every tile still above `target_tile_err` to the level pilot_spp << j its error predicts (at most `spp_count` per pixel), one
        render per group of tiles that share a move.  Into fresh host arrays; returns a dict: rgbw, m2, err (the error map), tile_spp,
        level_log ((max_rounds + 1, tiles): the level of every tile after the pilot and after each round), summary, stats."""
        return self._render_allocated_host(0, target_tile_err, (None, None, None), pilot_spp, max_rounds, headroom, spp_count, spp_begin, count_traversal, seed_mode, tile_mod, {})

    def render_allocated_denoised_host(self, target_tile_err, albedo=None, normal=None, depth=None, pilot_spp=16, max_rounds=3, headroom=1.0, spp_count=None,
                                       spp_begin=0, count_traversal=False, seed_mode=capi.SEED_PER_SAMPLE, tile_mod=1, **params):
        """render_allocated_host with the levels set on the error of the DENOISED frame (render_adaptive_denoised_host's metric): the
        dict also holds rgb, var, wsum -- denoise_var of the frames as they are left --, and err is the denoised error map."""
        return self._render_allocated_host(1, target_tile_err, (albedo, normal, depth), pilot_spp, max_rounds, headroom, spp_count, spp_begin, count_traversal, seed_mode, tile_mod, params)

    # -- film_order = reference shared out: rows of 32x32 blocks (include/nori_hip.h: nori_hip_render_block_rows) --
    def block_rows(self) -> int:
        """rows of 32x32 blocks (NORI_BLOCK_SIZE) in the frame"""
        return (self.scene.camera.height + 31) // 32

    def block_acc_floats(self) -> int:
        n = C.c_size_t(0)
        self._check(self._lib.nori_hip_block_acc_floats(self._h, C.byref(n)), "block_acc_floats")
        return int(n.value)

    def render_block_rows_into(self, acc_tensor, row_begin, row_count, spp_count=None, spp_begin=0, stream=None, count_traversal=False):
        """Block rows [row_begin, row_begin + row_count) in the reference's summation order: their blocks' accumulators are written
        into `acc_tensor` (CUDA float32, block_acc_floats() elements, zeroed by the caller; other blocks untouched)."""
        assert acc_tensor.is_cuda and acc_tensor.is_contiguous() and acc_tensor.numel() == self.block_acc_floats()
        spp = self.scene.sample_count if spp_count is None else spp_count
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        p = self._params(spp_begin, spp, 1, 0, count_traversal, raw, False)
        st = capi.RenderStats()
        self._check(self._lib.nori_hip_render_block_rows(self._h, C.byref(p), int(row_begin), int(row_count), C.c_void_p(acc_tensor.data_ptr()), C.byref(st)), "render_block_rows")
        return st.as_dict()

    def resolve_blocks(self, acc_tensor, rgbw_tensor, stream=None):
        """ImageBlock::put(ImageBlock&) of every block in BlockGenerator's order: adds into the RGBW frame tensor."""
        assert acc_tensor.is_cuda and acc_tensor.numel() == self.block_acc_floats()
        assert rgbw_tensor.is_cuda and rgbw_tensor.is_contiguous() and tuple(rgbw_tensor.shape) == tuple(self.frame_shape())
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._lib.nori_hip_resolve_blocks(self._h, C.c_void_p(acc_tensor.data_ptr()), C.c_void_p(rgbw_tensor.data_ptr()), raw), "resolve_blocks")
        return rgbw_tensor

    def develop(self, rgbw_tensor, stream=None):
        """ImageBlock::toBitmap on the device: (H, W, 3) torch tensor."""
        import torch
        c = self.scene.camera
        rgb = torch.empty((c.height, c.width, 3), dtype=torch.float32, device=rgbw_tensor.device)
        raw = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._lib.nori_hip_develop(self._h, C.c_void_p(rgbw_tensor.data_ptr()), C.c_void_p(rgb.data_ptr()), raw), "develop")
        return rgb


class DeviceGroup:
    """All GPUs of a node behind one call (nori_hip_group_*, include/nori_hip.h): the render loop of src/main.cpp:78-119
    with the image blocks shared out over devices instead of TBB workers and ImageBlock::put(ImageBlock&) as one merge."""
    SPLIT = {"tile": 0, "sample": 1}
    MERGE = {"reduce": 0, "gather": 1}

    def __init__(self, devices):
        self._lib = capi.load_hip()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._lib.nori_hip_group_create(devs, len(devices), C.byref(h))
        if rc != 0:
            msg = self._lib.nori_hip_group_last_error(None)
            raise NoriError(f"nori_hip_group_create({list(devices)}) failed: {capi.STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")
        self._h = h
        self.scene: Optional[Scene] = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nori_hip_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.nori_hip_group_last_error(self._h)
            raise NoriError(f"{what}: {capi.STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    @property
    def size(self) -> int:
        return int(self._lib.nori_hip_group_size(self._h))

    @property
    def transport(self) -> str:
        return self._lib.nori_hip_group_transport(self._h).decode()

    @property
    def warning(self) -> str:
        """"" or why the merge runs over peer copies although RCCL was wanted."""
        return self._lib.nori_hip_group_warning(self._h).decode()

    def engines(self):
        """nori_render_stats::engine of every device's share of the last frame."""
        out = (C.c_uint32 * self.size)()
        n = self._lib.nori_hip_group_engines(self._h, out, self.size)
        return [int(out[k]) for k in range(max(n, 0))]

    def upload(self, scene: Scene, builder: int = 0):
        desc, keep = scene.c_desc()
        self._check(self._lib.nori_hip_group_upload_scene(self._h, C.byref(desc), int(builder)), "group_upload_scene")
        del keep
        self.scene = scene
        if scene.camera.aperture_radius > 0:
            self.set_lens(scene.camera.aperture_radius, scene.camera.focus_distance)
        if getattr(scene, "environment", None) is not None:
            self.set_environment(scene.environment)
        if getattr(scene, "medium", None) is not None:
            self.set_medium(scene.medium)
        if getattr(scene, "lights", None):
            self.set_lights(scene.lights)
        return self

    def set_lights(self, lights):
        """Renderer.set_lights on every device of the group."""
        from .scene import light_array
        lights = list(lights) if lights is not None else []
        self._check(self._lib.nori_hip_group_set_lights(self._h, len(lights), light_array(lights)), "group_set_lights")
        return self

    def set_medium(self, medium):
        """Renderer.set_medium on every device of the group."""
        from .scene import GridMedium
        if isinstance(medium, GridMedium):
            return self.set_grid_medium(medium)
        d = medium.desc() if medium is not None else None
        self._check(self._lib.nori_hip_group_set_medium(self._h, C.byref(d) if d is not None else None), "group_set_medium")
        return self

    def set_grid_medium(self, medium):
        """Renderer.set_grid_medium on every device of the group."""
        d = medium.desc() if medium is not None else None
        self._check(self._lib.nori_hip_group_set_grid_medium(self._h, C.byref(d) if d is not None else None), "group_set_grid_medium")
        return self

    def set_environment(self, env):
        """Renderer.set_environment on every device of the group."""
        d = env.desc() if env is not None else None
        self._check(self._lib.nori_hip_group_set_environment(self._h, C.byref(d) if d is not None else None), "group_set_environment")
        return self

    def set_lens(self, radius: float, focus_distance: float = 1.0):
        """Renderer.set_lens on every device of the group."""
        self._check(self._lib.nori_hip_group_set_lens(self._h, float(radius), float(focus_distance)), "group_set_lens")
        return self

    def set_option(self, key: str, value) -> None:
        for i in range(self.size):
            ctx = self._lib.nori_hip_group_ctx(self._h, i)
            if self._lib.nori_hip_set_option(ctx, key.encode(), str(value).encode()) != 0:
                raise NoriError(f"set_option({key}) on group member {i}: {self._lib.nori_hip_last_error(ctx).decode()}")

    def render_host(self, split="tile", merge="reduce", spp_count=None, spp_begin=0, count_traversal=False):
        """(rgbw, stats dict, merge ms): the merged frame of all devices."""
        c = self.scene.camera
        b = self._lib.nori_hip_border_size(self._lib.nori_hip_group_ctx(self._h, 0))
        spp = self.scene.sample_count if spp_count is None else spp_count
        p = Renderer._params(spp_begin, spp, 1, 0, count_traversal, None)
        rgbw = np.zeros((c.height + 2 * b, c.width + 2 * b, 4), np.float32)
        st = capi.RenderStats()
        ms = C.c_float(0.0)
        self._check(self._lib.nori_hip_group_render_host(self._h, C.byref(p), self.SPLIT[split], self.MERGE[merge], c.width, c.height,
                                                         ptr(rgbw), C.byref(st), C.byref(ms)), "group_render_host")
        return rgbw, st.as_dict(), float(ms.value)


def develop_host(rgbw: np.ndarray, border: int) -> np.ndarray:
    """ImageBlock::toBitmap (src/block.cpp:45-51) for a host RGBW frame.  Pure
    reshaping/division of an already rendered frame (output side, not the hot path)."""
    h, w = rgbw.shape[0] - 2 * border, rgbw.shape[1] - 2 * border
    core = rgbw[border:border + h, border:border + w]
    wgt = core[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        rgb = np.where(wgt != 0, core[..., :3] / wgt, np.float32(0))
    return rgb.astype(np.float32)


def develop_features_host(frames: dict, border: int) -> dict:
    """The decode of include/nori_hip.h (nori_hip_render_features) for host feature frames, without the border, float32:
    "albedo" (H, W, 3) = rgb / W; "normal" (H, W, 3) = 2 rgb / W - 1, not renormalised; "depth" (H, W, 3) = (mean distance over
    the hits R / B, coverage B / W, mean squared distance over the hits G / B).  Each quotient is 0 where its divisor is <= 0."""
    def core(a):
        h, w = a.shape[0] - 2 * border, a.shape[1] - 2 * border
        return np.asarray(a, np.float32)[border:border + h, border:border + w]

    def quot(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, num / den, np.float32(0)).astype(np.float32)

    out = {}
    if "albedo" in frames:
        c = core(frames["albedo"])
        out["albedo"] = quot(c[..., :3], c[..., 3:4])
    if "normal" in frames:
        c = core(frames["normal"])
        out["normal"] = np.where(c[..., 3:4] > 0, np.float32(2) * quot(c[..., :3], c[..., 3:4]) - np.float32(1), np.float32(0)).astype(np.float32)
    if "depth" in frames:
        c = core(frames["depth"])
        out["depth"] = np.stack([quot(c[..., 0], c[..., 2]), quot(c[..., 2], c[..., 3]), quot(c[..., 1], c[..., 2])], axis=-1)
    return out
