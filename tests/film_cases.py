"""The film configurations shared by tests/test_film_reference_cpu.py and tests/test_gpu_film.py: frames, filters and
sample counts chosen for the branch of nori_amd/csrc/device/film.hip each one reaches (the reference-order kernel stages
a source pixel's samples 32 at a time, 16 once a filter has more than 11 taps, and adds them four at a time), and per
configuration the oracle's single-threaded frame and binary64 film, computed once per process."""
from __future__ import annotations

import functools

from nori_amd.scene import Bsdf, RFilter
from tests import scenes
from tests.backends import Oracle

# name: (width, height, filter, samples per pixel)                             what it reaches
ROWS = {
    "a-one-past-a-chunk": (45, 37, RFilter("gaussian"), 33),                   # one sample past a chunk of 32
    "b-two-chunks-and-6": (45, 37, RFilter("gaussian"), 70),                   # two chunks + a remainder of 6 (unroll 4 + 2)
    "c-tent-one-chunk": (33, 17, RFilter("tent"), 32),                         # exactly one chunk; weights that do not vanish at the edge
    "d-border5": (45, 37, RFilter("gaussian", radius=5.2, stddev=1.3), 34),    # 11 taps, chunk 32, the largest LDS request
    "e-border6": (45, 37, RFilter("gaussian", radius=6.0, stddev=1.5), 17),    # chunk 16, one past it
    "f-border8": (45, 37, RFilter("gaussian", radius=8.4, stddev=2.1), 20),    # 17 taps, four accumulator slots per thread
    "g-frame-inside-border": (5, 3, RFilter("gaussian", radius=8.4, stddev=2.1), 40),      # frame smaller than the border
    "h-one-pixel": (1, 1, RFilter("gaussian"), 40),                            # one live lane per tile
    "i-mitchell": (45, 37, RFilter("mitchell", radius=4.0), 9),                # negative lobes (abs_sum != sum)
    "j-box": (45, 37, RFilter("box"), 300),                                    # W is an integer count
    "k-1spp": (45, 37, RFilter("gaussian"), 1),                                # fewer samples than n_parts: empty parts
    "k-3spp": (45, 37, RFilter("gaussian"), 3),
}

def cornell(width, height, spp, rfilter, integrator="path_mis", radiance=None):
    """The Cornell box with a mirror and a glass sphere; `radiance` replaces the light's (20, 20, 20)."""
    sc = scenes.cornell_box(width, height, spp, integrator, sphere_bsdfs=[Bsdf("mirror"), Bsdf("dielectric")], rfilter=rfilter)
    if radiance is not None:
        light = [m for m in sc.meshes if m.name == "light"]
        assert len(light) == 1
        light[0].radiance = tuple(float(v) for v in radiance)
    return sc


def row_scene(name):
    w, h, rf, spp = ROWS[name]
    return cornell(w, h, spp, rf)


class FilmReference:
    """Of one scene: the oracle's frame in the reference's order (threads = 1) with its stats, and the binary64 film."""

    def __init__(self, sc, **params):
        o = Oracle(sc, use_bvh=True)
        self.scene, self.border = sc, o.border
        self.frame, self.stats = o.render_host(threads=1, **params)
        self.total, self.abs_total, self.terms, st64 = o.render_f64(threads=1, **params)
        assert all(st64[k] == self.stats[k] for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays")), (st64, self.stats)
        self.frame.setflags(write=False); self.total.setflags(write=False); self.abs_total.setflags(write=False); self.terms.setflags(write=False)
        o.close()

    @property
    def film(self):
        return self.total, self.abs_total, self.terms


@functools.lru_cache(maxsize=None)
def row_reference(name) -> FilmReference:
    return FilmReference(row_scene(name))
