"""The depth-of-field scene of tests/test_lens_cpu.py and tests/test_gpu_lens.py, and how the blur of an edge is counted.

Camera at the origin looking down +z (identity cameraToWorld), 96 x 40, horizontal field of view 40 degrees, focus distance F = 4.
Two quads facing the camera, each in its own half of the frame, each ending in a vertical edge 18.5 pixels from the frame's centre
(the middle of a pixel column, so the in-focus edge makes exactly one column partial):
    near  in the focal plane z = F,   x >= +18.5 p          (p: the width of a pixel on the focal plane)
    far   at depth z = 2 F,           x <= -18.5 p * 2      (the same angle on the other side)
Both reach far beyond the frame in y and on their outer side, so the only edges in view are the two vertical ones; 37 pixels lie
between them, three times the blur, so no ray bound for the far quad can be stopped by the near one.

A point at depth z is spread, on the focal plane, over a circle of diameter 2 R |z - F| / z: for z = 2 F that is R.  With
R = 0.36 the circle of confusion of the far edge is c = R / p = 11.87 pixels.
"""
from __future__ import annotations

import math

import numpy as np

from nori_amd.scene import Bsdf, Camera, Integrator, Mesh, RFilter, Scene
from tests import scenes

W, H, FOV, F, R, SPP = 96, 40, 40.0, 4.0, 0.36, 64
PIXEL = 2.0 * F * math.tan(math.radians(FOV) / 2.0) / W      # width of a pixel on the focal plane
EDGE = 18.5 * PIXEL
COC_PIXELS = R / PIXEL                                       # 2 R |2F - F| / (2F) = R, in pixels of the focal plane


def scene(integrator="normals"):
    big = 40.0
    v, f = scenes.quad((EDGE, -big, F), (big, -big, F), (big, big, F), (EDGE, big, F))
    near = Mesh(v, f, bsdf=Bsdf("diffuse", (0.7, 0.7, 0.7)), name="near")
    v, f = scenes.quad((-big, -big, 2 * F), (-2 * EDGE, -big, 2 * F), (-2 * EDGE, big, 2 * F), (-big, big, 2 * F))
    far = Mesh(v, f, bsdf=Bsdf("diffuse", (0.3, 0.5, 0.7)), name="far")
    return Scene([near, far], Camera(W, H, FOV), RFilter("box"), Integrator(integrator), SPP)


def analytic_hits(o, d):
    """(near, far) bool per ray: which quad the ray o + t d meets first (ray-plane, float64)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    xn = o[:, 0] + (F - o[:, 2]) / d[:, 2] * d[:, 0]
    xf = o[:, 0] + (2 * F - o[:, 2]) / d[:, 2] * d[:, 0]
    near = xn >= np.float32(EDGE)
    far = ~near & (xf <= np.float32(-2 * EDGE))
    return near, far


def partial_columns(cover):
    """cover: (W,) coverage of a quad per pixel column (hits / samples over all rows).  The number of columns strictly between
    0 and 1."""
    cover = np.asarray(cover, np.float64)
    return int(((cover > 0) & (cover < 1)).sum())


def edge_counts(cover_near, cover_far):
    return partial_columns(cover_near), partial_columns(cover_far)


def assert_blur(n_near, n_far, lens: bool):
    """The bounds of the issue: with c the geometric circle of confusion in pixels, c / 2 <= n <= c + 3 for the far edge and
    n <= 2 for the edge in focus; without a lens n <= 2 for both."""
    assert n_near <= 2, n_near
    if lens:
        assert COC_PIXELS / 2 <= n_far <= COC_PIXELS + 3, (n_far, COC_PIXELS)
    else:
        assert n_far <= 2, n_far
