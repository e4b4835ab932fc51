"""numpy float32 restatement of the albedo texture lookup (include/nori_hip.h, nori_texture_desc; rt_texture.h) and helpers
that build textured test scenes.  Every operation is a float32 operation in the order the header states, so the results
equal the device's bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32


def lookup(tex, uv) -> np.ndarray:
    """(n, 3) float32: texture `tex` (nori_amd.scene.Texture) at the (n, 2) texture coordinates uv."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        s = uv[:, 0] * F(tex.uscale) + F(tex.uoffset)
        t = uv[:, 1] * F(tex.vscale) + F(tex.voffset)
        s = np.where(np.abs(s) < np.inf, s, F(0)).astype(F)
        t = np.where(np.abs(t) < np.inf, t, F(0)).astype(F)
        if tex.kind == "checkerboard":
            ps = np.floor(s) - F(2) * np.floor(s * F(0.5))
            pt = np.floor(t) - F(2) * np.floor(t * F(0.5))
            return np.where((ps == pt)[:, None], np.asarray(tex.color0, F), np.asarray(tex.color1, F)).astype(F)
        clamp = tex.wrap == "clamp"
        wrap = (lambda x: np.minimum(np.maximum(x, F(0)), F(1))) if clamp else (lambda x: x - np.floor(x))
        s = wrap(s)
        t = F(1) - wrap(t)
        img = np.asarray(tex.texels, F)
        h, w = img.shape[:2]
        if tex.filter == "nearest":
            i = np.minimum((s * F(w)).astype(np.int64), w - 1)
            j = np.minimum((t * F(h)).astype(np.int64), h - 1)
            return img[j, i]
        idx = (lambda k, n: np.clip(k, 0, n - 1)) if clamp else (lambda k, n: np.mod(k, n))
        x, y = s * F(w) - F(0.5), t * F(h) - F(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        i1, j1 = idx(i0 + 1, w), idx(j0 + 1, h)
        i0, j0 = idx(i0, w), idx(j0, h)
        lerp = lambda a, b, f: a + f * (b - a)
        top = lerp(img[j0, i0], img[j0, i1], fx)
        bot = lerp(img[j1, i0], img[j1, i1], fx)
        return lerp(top, bot, fy).astype(F)


def grid_mesh_cells(corner, e1, e2, n):
    """n x n cells of the parallelogram corner + a e1 + b e2 (a, b in [0, 1]), two triangles each with vertices of their own:
    (positions (6 n^2, 3), indices (2 n^2, 3), cell centre (a, b) per triangle)."""
    c, e1, e2 = (np.asarray(v, np.float32) for v in (corner, e1, e2))
    pos, centres = [], []
    for i in range(n):
        for j in range(n):
            p = lambda a, b: c + F(a / n) * e1 + F(b / n) * e2
            p00, p10, p11, p01 = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
            pos += [p00, p10, p11, p00, p11, p01]
            centres += [((i + 0.5) / n, (j + 0.5) / n)] * 2
    pos = np.asarray(pos, np.float32)
    return pos, np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3), np.asarray(centres, np.float32)
