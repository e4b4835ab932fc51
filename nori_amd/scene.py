"""Flattened scene (`nori_scene_desc`) held in numpy arrays.

This is the data format on the caller's side of the C ABI: what the C++ host
(`libnori_host.so`, which parses Nori's XML/OBJ) hands over, what the `.npz`
fixtures under tests/golden/ store, and what `Renderer.upload` consumes.
Field names follow the reference's plugin parameters (src/diffuse.cpp:19,
src/microfacet.cpp:17-36, src/perspective.cpp:22-39, src/rfilter.cpp).
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _capi as capi


@dataclass
class Bsdf:
    type: str = "diffuse"
    albedo: tuple = (0.5, 0.5, 0.5)        # diffuse albedo / microfacet kd
    alpha: float = 0.1
    int_ior: float = 1.5046
    ext_ior: float = 1.000277

    @property
    def ks(self) -> float:                  # src/microfacet.cpp:35
        return float(np.float32(1.0) - np.float32(max(np.float32(x) for x in self.albedo)))

    def desc(self) -> capi.BsdfDesc:
        d = capi.BsdfDesc()
        d.type = capi.BSDF_NAMES[self.type]
        d.albedo[:] = [float(x) for x in self.albedo]
        d.alpha, d.int_ior, d.ext_ior = self.alpha, self.int_ior, self.ext_ior
        d.ks = self.ks if self.type == "microfacet" else 0.0
        return d


@dataclass
class Texture:
    """An albedo texture of a diffuse BSDF (nori_texture_desc in include/nori_hip.h, which states the lookup)."""
    kind: str = "image"                     # "image" | "checkerboard"
    texels: Optional[np.ndarray] = None     # image: (H, W, 3) float32 linear RGB, row 0 = the top row
    filter: str = "bilinear"                # "nearest" | "bilinear"
    wrap: str = "repeat"                    # "repeat" | "clamp"
    uscale: float = 1.0
    vscale: float = 1.0
    uoffset: float = 0.0
    voffset: float = 0.0
    color0: tuple = (0.4, 0.4, 0.4)         # checkerboard
    color1: tuple = (0.2, 0.2, 0.2)

    def __post_init__(self):
        if self.texels is not None:
            self.texels = np.ascontiguousarray(self.texels, dtype=np.float32)
            assert self.texels.ndim == 3 and self.texels.shape[2] == 3, "texels: (H, W, 3)"

    def params(self) -> dict:
        return {"kind": self.kind, "filter": self.filter, "wrap": self.wrap, "uscale": float(self.uscale), "vscale": float(self.vscale),
                "uoffset": float(self.uoffset), "voffset": float(self.voffset), "color0": list(map(float, self.color0)),
                "color1": list(map(float, self.color1))}

    def desc(self) -> capi.TextureDesc:
        d = capi.TextureDesc()
        d.type = capi.TEXTURE_NAMES[self.kind]
        if self.texels is not None:
            d.height, d.width = int(self.texels.shape[0]), int(self.texels.shape[1])
            d.texels = self.texels.ctypes.data_as(C.POINTER(C.c_float))
        d.filter = capi.TEXTURE_FILTER_NAMES[self.filter]
        d.wrap = capi.TEXTURE_WRAP_NAMES[self.wrap]
        d.uscale, d.vscale, d.uoffset, d.voffset = self.uscale, self.vscale, self.uoffset, self.voffset
        d.color0[:] = [float(x) for x in self.color0]
        d.color1[:] = [float(x) for x in self.color1]
        return d


@dataclass
class Environment:
    """An environment-map emitter (nori_env_desc in include/nori_hip.h, which states the lookup, the density and the sampling).
    Not part of nori_scene_desc: Renderer.upload applies it with nori_hip_set_environment."""
    texels: np.ndarray                      # (N, N, 3) float32 linear RGB, OCTAHEDRAL layout: texels[j, i] is column i of row j
    scale: tuple = (1.0, 1.0, 1.0)
    to_world: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=np.float32))      # rotation, world = M local

    def __post_init__(self):
        self.texels = np.ascontiguousarray(self.texels, dtype=np.float32)
        assert self.texels.ndim == 3 and self.texels.shape[0] == self.texels.shape[1] and self.texels.shape[2] == 3, "texels: (N, N, 3)"
        self.to_world = np.ascontiguousarray(self.to_world, dtype=np.float32).reshape(3, 3)

    def desc(self) -> capi.EnvDesc:
        """The ctypes struct; it borrows self.texels."""
        d = capi.EnvDesc()
        d.size = int(self.texels.shape[0])
        d.texels = self.texels.ctypes.data
        d.scale[:] = [float(x) for x in self.scale]
        d.to_world[:] = [float(x) for x in self.to_world.reshape(9)]
        return d


@dataclass
class Medium:
    """The homogeneous participating medium of a scene (nori_medium_desc in include/nori_hip.h, which states every operation): it
    fills all space.  Not part of nori_scene_desc: Renderer.upload applies it with nori_hip_set_medium."""
    sigma_t: float                          # grey extinction, 1e-4 .. 1e4
    albedo: tuple = (1.0, 1.0, 1.0)         # single-scattering albedo, each 0 .. 1
    g: float = 0.0                          # Henyey-Greenstein asymmetry, |g| <= 0.99; > 0 scatters forward

    def desc(self) -> capi.MediumDesc:
        d = capi.MediumDesc()
        d.sigma_t = float(self.sigma_t)
        d.albedo[:] = [float(x) for x in self.albedo]
        d.g = float(self.g)
        return d


@dataclass(eq=False)
class GridMedium:
    """The grid medium of a scene (nori_grid_medium_desc in include/nori_hip.h, which states every operation): a box of voxels of
    piecewise-constant density, vacuum outside it.  Accepted as Scene.medium in place of a Medium: Renderer.upload applies it with
    nori_hip_set_grid_medium."""
    rho: np.ndarray                         # (nz, ny, nx) float32 densities, each finite and >= 0: x fastest in memory
    bmin: tuple = (0.0, 0.0, 0.0)           # the box, world space
    bmax: tuple = (1.0, 1.0, 1.0)
    sigma_scale: float = 1.0                # a voxel's extinction is sigma_scale rho: 0, or 1e-4 .. 1e4
    albedo: tuple = (1.0, 1.0, 1.0)         # single-scattering albedo, each 0 .. 1
    g: float = 0.0                          # Henyey-Greenstein asymmetry, |g| <= 0.99; > 0 scatters forward

    def __post_init__(self):
        self.rho = np.ascontiguousarray(self.rho, dtype=np.float32)
        assert self.rho.ndim == 3, "rho: (nz, ny, nx)"
        self.bmin, self.bmax, self.albedo = tuple(map(float, self.bmin)), tuple(map(float, self.bmax)), tuple(map(float, self.albedo))

    def __eq__(self, other):
        return (isinstance(other, GridMedium) and self.rho.shape == other.rho.shape and self.rho.tobytes() == other.rho.tobytes() and
                (self.bmin, self.bmax, self.sigma_scale, self.albedo, self.g) == (other.bmin, other.bmax, other.sigma_scale, other.albedo, other.g))

    def desc(self) -> capi.GridMediumDesc:
        """The ctypes struct; it borrows self.rho."""
        d = capi.GridMediumDesc()
        d.rho = self.rho.ctypes.data
        d.nz, d.ny, d.nx = (int(x) for x in self.rho.shape)
        d.bmin[:], d.bmax[:] = self.bmin, self.bmax
        d.sigma_scale = float(self.sigma_scale)
        d.albedo[:] = self.albedo
        d.g = float(self.g)
        return d


@dataclass
class Light:
    """A delta light (nori_light_desc in include/nori_hip.h, which states every operation): "point", "spot" or "directional".
    Not part of nori_scene_desc: Renderer.upload applies Scene.lights with nori_hip_set_lights."""
    type: str
    position: tuple = (0.0, 0.0, 0.0)       # point, spot
    direction: tuple = (0.0, 0.0, 0.0)      # spot: the axis it shines along; directional: the direction the light travels
    intensity: tuple = (1.0, 1.0, 1.0)      # point, spot: radiant intensity (W/sr); directional: irradiance
    cos_inner: float = 0.0                  # spot: full intensity where the cosine to the axis is >= cos_inner,
    cos_outer: float = 0.0                  # none where it is <= cos_outer

    def desc(self) -> capi.LightDesc:
        d = capi.LightDesc()
        d.type = capi.LIGHT_TYPES.index(self.type)
        d.position[:] = [float(x) for x in self.position]
        d.direction[:] = [float(x) for x in self.direction]
        d.intensity[:] = [float(x) for x in self.intensity]
        d.cos_inner, d.cos_outer = float(self.cos_inner), float(self.cos_outer)
        return d

    @staticmethod
    def from_desc(d: capi.LightDesc) -> "Light":
        return Light(capi.LIGHT_TYPES[d.type], tuple(float(x) for x in d.position), tuple(float(x) for x in d.direction),
                     tuple(float(x) for x in d.intensity), float(d.cos_inner), float(d.cos_outer))


def light_array(lights):
    """the nori_light_desc array of a list of Light (None for an empty list)"""
    if not lights:
        return None
    arr = (capi.LightDesc * len(lights))()
    for k, l in enumerate(lights):
        arr[k] = l.desc()
    return arr


@dataclass
class Mesh:
    positions: np.ndarray                   # (nV, 3) float32, world space
    indices: np.ndarray                     # (nF, 3) uint32
    normals: Optional[np.ndarray] = None    # (nV, 3) float32
    texcoords: Optional[np.ndarray] = None  # (nV, 2) float32
    bsdf: Bsdf = field(default_factory=Bsdf)
    radiance: Optional[tuple] = None        # area emitter if not None
    name: str = ""
    albedo_texture: Optional[int] = None    # index into Scene.textures (0-based here, 1-based in nori_mesh_desc); diffuse only

    def __post_init__(self):
        self.positions = np.ascontiguousarray(self.positions, dtype=np.float32).reshape(-1, 3)
        self.indices = np.ascontiguousarray(self.indices, dtype=np.uint32).reshape(-1, 3)
        if self.normals is not None:
            self.normals = np.ascontiguousarray(self.normals, dtype=np.float32).reshape(-1, 3)
        if self.texcoords is not None:
            self.texcoords = np.ascontiguousarray(self.texcoords, dtype=np.float32).reshape(-1, 2)


@dataclass
class Camera:
    width: int = 1280
    height: int = 720
    fov: float = 30.0
    near_clip: float = 1e-4
    far_clip: float = 1e4
    to_world: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    # thin lens (include/nori_hip.h, "Thin-lens camera"): radius 0 is the pinhole.  Not part of nori_camera_desc: Renderer.upload
    # applies them with nori_hip_set_lens
    aperture_radius: float = 0.0
    focus_distance: float = 1.0


@dataclass
class RFilter:
    type: str = "gaussian"
    radius: float = 2.0
    stddev: float = 0.5
    B: float = 1.0 / 3.0
    C: float = 1.0 / 3.0


@dataclass
class Integrator:
    type: str = "path_mis"
    position: tuple = (0.0, 0.0, 0.0)
    energy: tuple = (0.0, 0.0, 0.0)


@dataclass
class Scene:
    meshes: List[Mesh] = field(default_factory=list)
    camera: Camera = field(default_factory=Camera)
    rfilter: RFilter = field(default_factory=RFilter)
    integrator: Integrator = field(default_factory=Integrator)
    sample_count: int = 1
    textures: List[Texture] = field(default_factory=list)
    environment: Optional[Environment] = None      # path_mats / path_ems / path_mis; applied after the upload
    medium: Optional[Medium] = None                # likewise; never together with an environment
    lights: List[Light] = field(default_factory=list)      # delta lights (path_ems / path_mis); applied after the upload

    # ------------------------------------------------------------ C view
    def c_desc(self):
        """(SceneDesc, keepalive): the ctypes struct plus the objects its pointers borrow."""
        n = len(self.meshes)
        arr = (capi.MeshDesc * max(n, 1))()
        keep = [arr]
        fp = C.POINTER(C.c_float)
        for i, m in enumerate(self.meshes):
            d = arr[i]
            d.n_vertices, d.n_triangles = m.positions.shape[0], m.indices.shape[0]
            d.positions = m.positions.ctypes.data_as(fp)
            d.normals = m.normals.ctypes.data_as(fp) if m.normals is not None else None
            d.texcoords = m.texcoords.ctypes.data_as(fp) if m.texcoords is not None else None
            d.indices = m.indices.ctypes.data_as(C.POINTER(C.c_uint32))
            d.bsdf = m.bsdf.desc()
            d.is_emitter = 1 if m.radiance is not None else 0
            d.radiance[:] = [float(x) for x in (m.radiance or (0, 0, 0))]
            d.albedo_texture = 0 if m.albedo_texture is None else int(m.albedo_texture) + 1
            keep.append(m)
        s = capi.SceneDesc()
        s.n_meshes = n
        s.meshes = C.cast(arr, C.POINTER(capi.MeshDesc))
        c = self.camera
        s.camera.width, s.camera.height = int(c.width), int(c.height)
        s.camera.fov, s.camera.near_clip, s.camera.far_clip = c.fov, c.near_clip, c.far_clip
        s.camera.to_world[:] = [float(x) for x in np.asarray(c.to_world, dtype=np.float32).reshape(16)]
        f = self.rfilter
        s.rfilter.type = capi.RFILTER_NAMES[f.type]
        s.rfilter.radius, s.rfilter.stddev, s.rfilter.B, s.rfilter.C = f.radius, f.stddev, f.B, f.C
        it = self.integrator
        s.integrator.type = capi.INTEGRATOR_NAMES[it.type]
        s.integrator.position[:] = [float(x) for x in it.position]
        s.integrator.energy[:] = [float(x) for x in it.energy]
        s.sample_count = int(self.sample_count)
        if self.textures:
            tarr = (capi.TextureDesc * len(self.textures))(*[t.desc() for t in self.textures])
            keep += [tarr] + list(self.textures)
            s.n_textures = len(self.textures)
            s.textures = C.cast(tarr, C.POINTER(capi.TextureDesc))
        return s, keep

    @property
    def n_triangles(self) -> int:
        return int(sum(m.indices.shape[0] for m in self.meshes))

    @property
    def border(self) -> int:
        f = self.rfilter
        r = 1.0 if f.type == "tent" else (0.5 if f.type == "box" else f.radius)
        return int(np.ceil(np.float32(r) - np.float32(0.5)))

    def frame_shape(self):
        b = self.border
        return (self.camera.height + 2 * b, self.camera.width + 2 * b, 4)

    # --------------------------------------------------------- (de)serialise
    def geometry_digest(self) -> str:
        """sha256 over everything a fixture stores as arrays (camera transform, per mesh V / F / N / UV)."""
        import hashlib
        h = hashlib.sha256()
        h.update(np.ascontiguousarray(self.camera.to_world, dtype=np.float32).tobytes())
        for m in self.meshes:
            for a in (m.positions, m.indices, m.normals, m.texcoords):
                h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
        if self.textures:      # (scenes without textures: the digest of before, which profiles and fixtures are keyed by)
            for t in self.textures:
                h.update(b"t-" if t.texels is None else b"t" + np.asarray(t.texels.shape, dtype=np.int64).tobytes() + t.texels.tobytes())
            h.update(np.asarray([-1 if m.albedo_texture is None else m.albedo_texture for m in self.meshes], dtype=np.int64).tobytes())
        return h.hexdigest()

    def save_npz(self, path: str, base: Optional[str] = None) -> None:
        """`base`: name of a fixture in the same directory with the same arrays (several shipped scenes differ in the integrator,
        the sample count or one BSDF only): the file then holds the parameters and the digest of the arrays, not the arrays."""
        meta = {
            "camera": {"width": self.camera.width, "height": self.camera.height, "fov": self.camera.fov,
                       "near_clip": self.camera.near_clip, "far_clip": self.camera.far_clip},
            "rfilter": vars(self.rfilter), "integrator": {"type": self.integrator.type,
                                                          "position": list(self.integrator.position),
                                                          "energy": list(self.integrator.energy)},
            "sample_count": self.sample_count,
            "meshes": [{"name": m.name, "bsdf": {"type": m.bsdf.type, "albedo": list(map(float, m.bsdf.albedo)),
                                                 "alpha": m.bsdf.alpha, "int_ior": m.bsdf.int_ior,
                                                 "ext_ior": m.bsdf.ext_ior},
                        "radiance": list(map(float, m.radiance)) if m.radiance is not None else None,
                        "normals": m.normals is not None, "texcoords": m.texcoords is not None,
                        **({"albedo_texture": m.albedo_texture} if m.albedo_texture is not None else {})}
                       for m in self.meshes],
        }
        if self.camera.aperture_radius > 0:      # (pinhole scenes: the file of before, key for key)
            meta["camera"].update(aperture_radius=float(self.camera.aperture_radius), focus_distance=float(self.camera.focus_distance))
        if self.textures:
            meta["textures"] = [dict(t.params(), texels=t.texels is not None) for t in self.textures]
        if self.environment is not None:      # (scenes without one: the file of before, key for key)
            meta["environment"] = {"scale": list(map(float, self.environment.scale))}
        if isinstance(self.medium, GridMedium):      # (likewise; the voxels are an array of their own)
            assert base is None, "a variant fixture (base=...) stores no arrays: save a scene with a grid medium whole"
            m = self.medium
            meta["grid_medium"] = {"bmin": list(m.bmin), "bmax": list(m.bmax), "sigma_scale": float(m.sigma_scale), "albedo": list(m.albedo), "g": float(m.g)}
        elif self.medium is not None:           # (likewise)
            meta["medium"] = {"sigma_t": float(self.medium.sigma_t), "albedo": list(map(float, self.medium.albedo)), "g": float(self.medium.g)}
        if self.lights:                       # (likewise)
            meta["lights"] = [{"type": l.type, "position": list(map(float, l.position)), "direction": list(map(float, l.direction)),
                               "intensity": list(map(float, l.intensity)), "cos_inner": float(l.cos_inner), "cos_outer": float(l.cos_outer)}
                              for l in self.lights]
        if base is not None:
            assert self.environment is None, "a variant fixture (base=...) stores no arrays: save a scene with an environment whole"
            assert not self.textures, "a variant fixture (base=...) stores no arrays: save a textured scene whole"
            meta["base"], meta["geometry_digest"] = base, self.geometry_digest()
            np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
            return
        arrays = {"to_world": np.asarray(self.camera.to_world, dtype=np.float32)}
        for i, m in enumerate(self.meshes):
            arrays[f"m{i}_V"] = m.positions
            arrays[f"m{i}_F"] = m.indices
            if m.normals is not None:
                arrays[f"m{i}_N"] = m.normals
            if m.texcoords is not None:
                arrays[f"m{i}_UV"] = m.texcoords
        for k, t in enumerate(self.textures):
            if t.texels is not None:
                arrays[f"t{k}_texels"] = t.texels
        if self.environment is not None:
            arrays["env_texels"], arrays["env_to_world"] = self.environment.texels, self.environment.to_world
        if isinstance(self.medium, GridMedium):
            arrays["grid_medium_rho"] = self.medium.rho
        arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(path, **arrays)

    @staticmethod
    def load_npz(path: str) -> "Scene":
        z = np.load(path)
        meta = json.loads(bytes(z["meta"]).decode())
        if "base" in meta:      # parameters of this scene over the arrays of another fixture (save_npz)
            import os
            sc = Scene.load_npz(os.path.join(os.path.dirname(os.path.abspath(path)), meta["base"] + ".npz"))
            assert len(sc.meshes) == len(meta["meshes"]), "variant fixture does not match its base"
            cam = sc.camera.to_world
            sc.camera = Camera(to_world=cam, **meta["camera"])
            sc.rfilter = RFilter(**meta["rfilter"])
            it = meta["integrator"]
            sc.integrator = Integrator(it["type"], tuple(it["position"]), tuple(it["energy"]))
            sc.sample_count = meta["sample_count"]
            for m, mm in zip(sc.meshes, meta["meshes"]):
                b = mm["bsdf"]
                m.bsdf = Bsdf(b["type"], tuple(b["albedo"]), b["alpha"], b["int_ior"], b["ext_ior"])
                m.radiance = tuple(mm["radiance"]) if mm["radiance"] is not None else None
                m.name = mm["name"]
            assert sc.geometry_digest() == meta["geometry_digest"], "variant fixture: the base fixture's arrays have changed"
            return sc
        sc = Scene()
        sc.camera = Camera(to_world=z["to_world"].astype(np.float32), **meta["camera"])
        sc.rfilter = RFilter(**meta["rfilter"])
        it = meta["integrator"]
        sc.integrator = Integrator(it["type"], tuple(it["position"]), tuple(it["energy"]))
        sc.sample_count = meta["sample_count"]
        for i, mm in enumerate(meta["meshes"]):
            b = mm["bsdf"]
            sc.meshes.append(Mesh(z[f"m{i}_V"], z[f"m{i}_F"],
                                  z[f"m{i}_N"] if mm["normals"] else None,
                                  z[f"m{i}_UV"] if mm["texcoords"] else None,
                                  Bsdf(b["type"], tuple(b["albedo"]), b["alpha"], b["int_ior"], b["ext_ior"]),
                                  tuple(mm["radiance"]) if mm["radiance"] is not None else None, mm["name"],
                                  mm.get("albedo_texture")))
        for k, tm in enumerate(meta.get("textures", [])):
            p = dict(tm)
            has_texels = p.pop("texels")
            p["color0"], p["color1"] = tuple(p["color0"]), tuple(p["color1"])
            sc.textures.append(Texture(texels=z[f"t{k}_texels"] if has_texels else None, **p))
        if "environment" in meta:
            sc.environment = Environment(z["env_texels"], tuple(meta["environment"]["scale"]), z["env_to_world"])
        if "medium" in meta:
            sc.medium = Medium(meta["medium"]["sigma_t"], tuple(meta["medium"]["albedo"]), meta["medium"]["g"])
        if "grid_medium" in meta:
            gm = meta["grid_medium"]
            sc.medium = GridMedium(z["grid_medium_rho"], tuple(gm["bmin"]), tuple(gm["bmax"]), gm["sigma_scale"], tuple(gm["albedo"]), gm["g"])
        for l in meta.get("lights", []):
            sc.lights.append(Light(l["type"], tuple(l["position"]), tuple(l["direction"]), tuple(l["intensity"]), l["cos_inner"], l["cos_outer"]))
        return sc
