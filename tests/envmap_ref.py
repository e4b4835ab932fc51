"""The environment-map emitter restated in numpy float32, operation by operation as include/nori_hip.h states it ("Environment-map
emitter"): the tables, the lookup, the density, the sampling -- vectorised (EnvRef) and as a scalar loop over single directions and
samples (eval_scalar, sample_scalar), which the CPU suite holds against each other and the GPU suite holds the device to, bit for
bit.  numpy rounds every float32 operation on its own (no contraction) and its / and sqrt are IEEE's, which is the arithmetic the
device code is written for (exact_div, exact_sqrt)."""
from __future__ import annotations

import numpy as np

F = np.float32
LUM = (F(0.212671), F(0.715160), F(0.072169))


def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + (ay * by + az * bz)


def _sgn(x):
    return np.where(x >= 0, F(1), F(-1)).astype(np.float32)


def _fold(px, py):
    return (F(1) - np.abs(py)) * _sgn(px), (F(1) - np.abs(px)) * _sgn(py)


def _cube(x, y, z):
    n = _dot(x, y, z, x, y, z)
    return n * np.sqrt(n)


def _cdf(w):
    """DiscretePDF over the last axis: sequential float32 sums in index order (np.add.accumulate is sequential), one division by the
    total where it is > 0; returns (cdf with a leading 0, totals)"""
    w = np.asarray(w, np.float32)
    acc = np.add.accumulate(w, axis=-1, dtype=np.float32)
    cdf = np.concatenate([np.zeros(w.shape[:-1] + (1,), np.float32), acc], axis=-1)
    tot = cdf[..., -1].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = cdf / tot[..., None]
    return np.where(tot[..., None] > 0, norm, cdf).astype(np.float32), tot


class EnvRef:
    def __init__(self, texels, scale=(1.0, 1.0, 1.0), to_world=np.eye(3)):
        self.texels = np.ascontiguousarray(texels, np.float32)
        self.n = int(self.texels.shape[0])
        assert self.texels.shape == (self.n, self.n, 3)
        self.scale = np.asarray(scale, np.float32)
        self.m = np.asarray(to_world, np.float32).reshape(3, 3)
        self.le = self.texels * self.scale                      # Le of texel [j, i]
        n, fn = self.n, F(self.n)
        c = (np.arange(n, dtype=np.float32) + F(0.5)) / fn      # texel centres
        u, v = np.meshgrid(c, c)                                # [j, i]: u varies with the column i, v with the row j
        px, py = u * F(2) - F(1), v * F(2) - F(1)
        pz = (F(1) - np.abs(px)) - np.abs(py)
        fx, fy = _fold(px, py)
        px, py = np.where(pz < 0, fx, px), np.where(pz < 0, fy, py)
        lum = (self.le[..., 0] * LUM[0] + self.le[..., 1] * LUM[1]) + self.le[..., 2] * LUM[2]
        self.weight = (lum / _cube(px, py, pz)).astype(np.float32)
        self.col_cdf, row_sum = _cdf(self.weight)               # (N, N + 1)
        self.row_cdf, _ = _cdf(row_sum)                         # (N + 1,)
        for a in (self.weight, self.col_cdf, self.row_cdf, self.le):
            assert a.dtype == np.float32
            a.setflags(write=False)

    # ---- direction -> (q, u, v) -> texel
    def dir_to_uv(self, d):
        d = np.asarray(d, np.float32).reshape(-1, 3)
        m = self.m
        l = [_dot(m[0, k], m[1, k], m[2, k], d[:, 0], d[:, 1], d[:, 2]) for k in range(3)]      # M^T d
        s = (np.abs(l[0]) + np.abs(l[1])) + np.abs(l[2])
        with np.errstate(invalid="ignore", divide="ignore"):      # (a zero vector is no direction: NaN, texel 0 after the clamp)
            q = [l[k] / s for k in range(3)]
        fx, fy = _fold(q[0], q[1])
        px, py = np.where(q[2] < 0, fx, q[0]), np.where(q[2] < 0, fy, q[1])
        return q, px * F(0.5) + F(0.5), py * F(0.5) + F(0.5)

    def texel_of(self, u, v):
        fn = F(self.n)
        with np.errstate(invalid="ignore"):
            i = np.clip(np.nan_to_num(u * fn).astype(np.int32), 0, self.n - 1)
            j = np.clip(np.nan_to_num(v * fn).astype(np.int32), 0, self.n - 1)
        return i, j

    def eval(self, d):
        """(Le (n, 3), pdf (n,), (i, j))"""
        q, u, v = self.dir_to_uv(d)
        i, j = self.texel_of(u, v)
        fn = F(self.n)
        p = (self.row_cdf[j + 1] - self.row_cdf[j]) * (self.col_cdf[j, i + 1] - self.col_cdf[j, i])
        pdf = (p * ((fn * fn) * F(0.25))) * _cube(*q)
        return self.le[j, i], pdf.astype(np.float32), (i, j)

    # ---- sampling
    @staticmethod
    def _pick(cdf, n, xi):
        """DiscretePDF::sample on each row of cdf (k, n + 1) with its own xi (k,): (index, reused sample)"""
        lo = (cdf < xi[:, None]).sum(axis=1)                    # std::lower_bound on a non-decreasing row: the count of entries < xi
        k = np.minimum(np.maximum(lo - 1, 0), n - 1)
        r = np.arange(cdf.shape[0])
        lo_v, den = cdf[r, k], cdf[r, k + 1] - cdf[r, k]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(den > 0, (xi - lo_v) / den, F(0.5)).astype(np.float32)
        return k, t

    def sample(self, xi):
        """(d (n, 3), Le, pdf, (i, j) picked by the CDFs)"""
        xi = np.asarray(xi, np.float32).reshape(-1, 2)
        n, fn = self.n, F(self.n)
        j, ty = self._pick(np.broadcast_to(self.row_cdf, (xi.shape[0], n + 1)), n, xi[:, 1])
        i, tx = self._pick(self.col_cdf[j], n, xi[:, 0])
        u, v = (i.astype(np.float32) + tx) / fn, (j.astype(np.float32) + ty) / fn
        px, py = u * F(2) - F(1), v * F(2) - F(1)
        pz = (F(1) - np.abs(px)) - np.abs(py)
        fx, fy = _fold(px, py)
        px, py = np.where(pz < 0, fx, px), np.where(pz < 0, fy, py)
        ln = np.sqrt(_dot(px, py, pz, px, py, pz))
        l = [px / ln, py / ln, pz / ln]
        m = self.m
        d = np.stack([_dot(m[k, 0], m[k, 1], m[k, 2], l[0], l[1], l[2]) for k in range(3)], axis=1).astype(np.float32)
        le, pdf, _ = self.eval(d)
        return d, le, pdf, (i, j)

    def texel_centre_dirs(self):
        """the local-frame unit directions of the texel centres, [j, i, 3] (float64: for quadrature and round trips)"""
        c = (np.arange(self.n) + 0.5) / self.n
        u, v = np.meshgrid(c, c)
        return uv_to_dir64(u, v)


def uv_to_dir64(u, v):
    px, py = 2 * u - 1, 2 * v - 1
    pz = 1 - np.abs(px) - np.abs(py)
    fx, fy = (1 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), (1 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0)
    px, py = np.where(pz < 0, fx, px), np.where(pz < 0, fy, py)
    p = np.stack([px, py, pz], axis=-1)
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


# ---------------------------------------------------------------- the scalar statement: one direction / one sample at a time
def _fold1(px, py):
    sx = F(1) if px >= 0 else F(-1)
    sy = F(1) if py >= 0 else F(-1)
    return (F(1) - abs(py)) * sx, (F(1) - abs(px)) * sy


def _cube1(x, y, z):
    n = x * x + (y * y + z * z)
    return n * np.sqrt(n)


def eval_scalar(env: EnvRef, d):
    m, n, fn = env.m, env.n, F(env.n)
    d = [F(x) for x in d]
    l = [m[0, k] * d[0] + (m[1, k] * d[1] + m[2, k] * d[2]) for k in range(3)]
    s = (abs(l[0]) + abs(l[1])) + abs(l[2])
    q = [l[k] / s for k in range(3)]
    px, py = q[0], q[1]
    if q[2] < 0:
        px, py = _fold1(px, py)
    u, v = px * F(0.5) + F(0.5), py * F(0.5) + F(0.5)
    i, j = min(max(int(u * fn), 0), n - 1), min(max(int(v * fn), 0), n - 1)
    p = (env.row_cdf[j + 1] - env.row_cdf[j]) * (env.col_cdf[j, i + 1] - env.col_cdf[j, i])
    pdf = (p * ((fn * fn) * F(0.25))) * _cube1(*q)
    return env.le[j, i], F(pdf), (i, j)


def _pick1(cdf, n, xi):
    lo, ln = 0, n + 1
    while ln > 0:                                   # std::lower_bound
        half = ln >> 1
        mid = lo + half
        if cdf[mid] < xi:
            lo, ln = mid + 1, ln - (half + 1)
        else:
            ln = half
    k = min(max(lo - 1, 0), n - 1)
    den = cdf[k + 1] - cdf[k]
    return k, ((xi - cdf[k]) / den if den > 0 else F(0.5))


def sample_scalar(env: EnvRef, xi):
    n, fn, m = env.n, F(env.n), env.m
    x, y = F(xi[0]), F(xi[1])
    j, ty = _pick1(env.row_cdf, n, y)
    i, tx = _pick1(env.col_cdf[j], n, x)
    u, v = (F(i) + tx) / fn, (F(j) + ty) / fn
    px, py = u * F(2) - F(1), v * F(2) - F(1)
    pz = (F(1) - abs(px)) - abs(py)
    if pz < 0:
        px, py = _fold1(px, py)
    ln = np.sqrt(px * px + (py * py + pz * pz))
    l = [px / ln, py / ln, pz / ln]
    d = np.array([m[k, 0] * l[0] + (m[k, 1] * l[1] + m[k, 2] * l[2]) for k in range(3)], np.float32)
    le, pdf, _ = eval_scalar(env, d)
    return d, le, pdf, (i, j)


# ---------------------------------------------------------------- maps and operands the suites share
def rotation(seed=5):
    """a rotation about all three axes, float32 (orthonormal to ~1e-7)"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def make_map(n, kind="random", seed=0):
    rng = np.random.default_rng(seed + 17 * n)
    t = rng.uniform(0.05, 2.0, (n, n, 3)).astype(np.float32)
    if kind == "zeros":                 # a third of the texels black -- texel (0, 0) among them, which xi = 0 selects --, and a whole black row if there is room
        t[rng.random((n, n)) < 0.33] = 0
        t[0, 0] = 0
        if n > 2:
            t[n // 2] = 0
        if not t.any():
            t[-1, -1] = 1
    elif kind == "range":               # 10^6 dynamic range
        t = (t * np.float32(10.0) ** rng.uniform(-3, 3, (n, n, 1))).astype(np.float32)
    elif kind == "contrast":            # a sun, a bright band, a dim rest
        t[:] = 0.02
        t[n // 3] = 1.5
        t[(2 * n) // 3, n // 4] = 400.0
    else:
        assert kind == "random"
    return t


def directions(n_random=4000, seed=1):
    """random unit directions, the six axes, and directions ON the seams z = 0, x = 0, y = 0 of the local frame (callers rotate them)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_random, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    phi = rng.uniform(0, 2 * np.pi, 300)
    c, s, z = np.cos(phi), np.sin(phi), np.zeros(300)
    seams = np.concatenate([np.stack([c, s, z], 1), np.stack([z, c, s], 1), np.stack([c, z, s], 1)])
    return np.concatenate([d, axes, seams]).astype(np.float32)


def samples(env: EnvRef, n_random=4000, seed=2):
    """random samples, 0, 1 - 2^-24, and every CDF boundary value with its float neighbours, in x against every row and in y"""
    rng = np.random.default_rng(seed)
    xi = [rng.random((n_random, 2), dtype=np.float32)]
    top = np.float32(1) - np.float32(2.0 ** -24)
    xi.append(np.array([(0, 0), (0, 0.5), (0.5, 0), (top, top), (top, 0.25), (0.25, top)], np.float32))
    def around(c):
        c = np.unique(np.asarray(c, np.float32).ravel())
        c = np.concatenate([c, np.nextafter(c, np.float32(-1)), np.nextafter(c, np.float32(2))])
        return c[(c >= 0) & (c < 1)]
    rows = around(env.row_cdf)
    xi.append(np.stack([np.full(rows.shape, 0.375, np.float32), rows], axis=1))
    # a column boundary matters in its own row: pair it with a y that selects that row (the row's middle in the row CDF)
    mid = ((env.row_cdf[:-1].astype(np.float64) + env.row_cdf[1:]) / 2).astype(np.float32)
    for j in range(env.n):
        if env.row_cdf[j + 1] > env.row_cdf[j]:
            cols = around(env.col_cdf[j])
            xi.append(np.stack([cols, np.full(cols.shape, mid[j], np.float32)], axis=1))
    return np.concatenate(xi).astype(np.float32)
