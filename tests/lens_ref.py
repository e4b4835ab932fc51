"""The thin-lens camera of include/nori_hip.h ("Thin-lens camera"), restated in numpy.

float32 (the default) evaluates the statement operation by operation: every numpy operation on float32 arrays is one correctly
rounded IEEE operation, there is no contraction, and the association of every sum is written out -- so the result is what
camera_sample_ray_lens (rt_trace.h) computes, bit for bit.  dtype=np.float64 evaluates the SAME formulas in binary64 from the
same inputs, for the property tests (do the rays of a film point meet on the focal plane?) and as the yardstick of the float32
evaluation's rounding error.

Two inputs are not recomputed here but taken from the oracle, because the statement takes them from existing operations:
  d      "exactly as camera_sample_ray today": the camera-space direction of the pinhole ray is what the oracle's sampleRay returns
         for the same camera with an identity cameraToWorld (1 * d.x + (0 * d.y + 0 * d.z) is d.x);
  disk   squareToUniformDisk(apertureSample), the oracle's warp with the pinned sine and cosine.
radius == 0 is not this arithmetic: it is the pinhole ray of the oracle's sampleRay.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from nori_amd import _capi as capi

from tests.backends import Oracle

#: roundings between the inputs (d, disk) and a component of the returned direction, counted along the longest chain:
#: F * invZ (invZ: 1, product: 1), pf (1), l (1), pf - l (1), the squared length (a product and two sums: 3), its root (1),
#: the quotient (1), the transform (a product and two sums: 3)
DIRECTION_ROUNDINGS = 14


def camera_space_directions(scene, pixel_samples):
    """(n, 3) float32: normalized(sampleToCamera * (x / w, y / h, 0)) of the scene's camera, and the pinhole's (mint, maxt)."""
    cam = dataclasses.replace(scene.camera, to_world=np.eye(4, dtype=np.float32))
    rays = Oracle(dataclasses.replace(scene, camera=cam)).sample_rays(pixel_samples)
    assert np.all(rays["o"] == 0)
    return rays["d"].copy()


def disk_points(aperture_samples):
    """(n, 2) float32: the oracle's squareToUniformDisk."""
    a = np.ascontiguousarray(aperture_samples, np.float32).reshape(-1, 2)
    return Oracle.warp("disk", a)[:, :2].copy()


def _div(a, b):
    """The device's quotient (rt_types.h, exact_div): correctly rounded, and -0 / b is +0 for b > 0."""
    assert np.all(b > 0)
    return a / b + a.dtype.type(0.0)


def lens_rays(scene, pixel_samples, aperture_samples, radius, focus_distance, dtype=np.float32):
    """dict of o (n, 3), d (n, 3), mint (n,), maxt (n,) in `dtype`, and for the property tests the camera-space quantities pf
    (the point on the focal plane), l (the point on the lens) and dl (the direction)."""
    T = np.dtype(dtype).type
    ps = np.ascontiguousarray(pixel_samples, np.float32).reshape(-1, 2)
    cam = scene.camera
    if not radius > 0:
        rays = Oracle(scene).sample_rays(ps)
        return {"o": rays["o"].astype(T), "d": rays["d"].astype(T), "mint": rays["mint"].astype(T), "maxt": rays["maxt"].astype(T)}
    R, F = T(np.float32(radius)), T(np.float32(focus_distance))
    near, far = T(np.float32(cam.near_clip)), T(np.float32(cam.far_clip))
    m = np.asarray(cam.to_world, np.float32).reshape(4, 4).astype(T)
    d = camera_space_directions(scene, ps).astype(T)
    disk = disk_points(aperture_samples).astype(T)
    assert disk.shape[0] == d.shape[0]
    one = T(1.0)

    inv_z = one / d[:, 2]
    pf = d * (F * inv_z)[:, None]
    l = np.stack([R * disk[:, 0], R * disk[:, 1], np.zeros(d.shape[0], T)], axis=1)
    v = pf - l
    z = v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    assert np.all(z > 0)
    dl = _div(v, np.sqrt(z)[:, None])
    # mat_point: ((m0 x + m1 y) + m2 z) + m3 * 1, then the division by w
    r = [((m[i, 0] * l[:, 0] + m[i, 1] * l[:, 1]) + m[i, 2] * l[:, 2]) + m[i, 3] * one for i in range(4)]
    o = np.stack([_div(r[i], r[3]) for i in range(3)], axis=1)
    # mat_vector: m0 x + (m1 y + m2 z)
    dw = np.stack([m[i, 0] * dl[:, 0] + (m[i, 1] * dl[:, 1] + m[i, 2] * dl[:, 2]) for i in range(3)], axis=1)
    inv_zl = one / dl[:, 2]
    out = {"o": o, "d": dw, "mint": near * inv_zl, "maxt": far * inv_zl, "pf": pf, "l": l, "dl": dl}
    assert all(a.dtype == np.dtype(dtype) for a in out.values())
    return out


def as_rays(r):
    """float32 lens_rays -> the nori_ray records the twins take."""
    rays = np.zeros(r["o"].shape[0], capi.RAY_DTYPE)
    for k in ("o", "d", "mint", "maxt"):
        assert r[k].dtype == np.float32
        rays[k] = r[k]
    return rays


def camera_samples(width, height, s, pcg32_floats=Oracle.pcg32_floats):
    """The four floats of camera sample s of every pixel, row-major (py * W + px): pcg32.seed(py * W + px, s), nextFloat x 4, from the
    oracle's pcg32 or the twin given (Renderer.pcg32_floats).  Returns ((H * W, 2) pixelSample, (H * W, 2) apertureSample)."""
    idx = np.arange(width * height, dtype=np.uint64)
    f = pcg32_floats(idx, np.full(idx.shape, s, np.uint64), 4)
    px, py = (idx % np.uint64(width)).astype(np.float32), (idx // np.uint64(width)).astype(np.float32)
    ps = np.stack([px + f[:, 0], py + f[:, 1]], axis=1).astype(np.float32)
    return ps, f[:, 2:4].copy()
