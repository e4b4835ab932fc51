"""What an environment map costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024,
the device-built tree) at 16 samples per pixel, in one process and one context, alternately without an environment and with a
512 x 512 sky (a gradient with a sun: three decades of range), on both engines.  With the environment the scene has two lights and
paths that leave the box collect the sky, so the render traces OTHER paths: the ray counts are printed beside the times, and the
comparison that isolates the kernels' own cost is time per ray.  Also timed: nori_hip_set_environment itself (the copy and the three
table kernels, synchronous) for N = 512 and N = 4096, and the operator twins on 2^20 directions / samples.
Per run: the wall time of an untimed call and a synchronize, and trace_ms / film_ms / kernel_ms of a second call with time_kernels
on.  Reported as median (min - max) over the runs: the spread is the yardstick for every comparison.
    python tools/env_cost.py [--runs 5] [--spp 16] [--json profiles/env_cost.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nori_amd.render import Renderer  # noqa: E402
from nori_amd.scene import Environment, Scene  # noqa: E402


def sky(n):
    """octahedral texels: brighter towards +y, a sun of 1000 x the zenith in one texel's neighbourhood"""
    c = (np.arange(n) + 0.5) / n
    u, v = np.meshgrid(c, c)
    px, py = 2 * u - 1, 2 * v - 1
    pz = 1 - np.abs(px) - np.abs(py)
    fx, fy = (1 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), (1 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0)
    px, py = np.where(pz < 0, fx, px), np.where(pz < 0, fy, py)
    d = np.stack([px, py, pz], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    up = np.maximum(d[..., 1], 0.0)
    sun = np.array([0.3, 0.8, 0.52]) / np.linalg.norm([0.3, 0.8, 0.52])
    t = np.stack([0.3 + 0.5 * up, 0.4 + 0.6 * up, 0.6 + 0.9 * up], -1) + 1000.0 * (d @ sun > 0.9995)[..., None]
    return t.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    envs = {"none": None, "sky512": Environment(sky(512))}
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")

    set_ms = {}
    for n in (512, 4096):
        e = Environment(sky(n))
        r.set_environment(e)      # warm-up: code objects
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r.set_environment(e)
            ts.append((time.perf_counter() - t0) * 1e3)
        set_ms[n] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
        print("set_environment", n, set_ms[n], flush=True)
    r.set_environment(envs["sky512"])
    rng = np.random.default_rng(0)
    xi = rng.random((1 << 20, 2), dtype=np.float32)
    d, _, _ = r.env_sample(xi)
    ops = {}
    for name, call in (("env_sample", lambda: r.env_sample(xi)), ("env_eval", lambda: r.env_eval(d))):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        ops[name] = {"n": 1 << 20, "wall_ms_with_copies": float(np.median(ts))}
        print(name, ops[name], flush=True)

    def render(engine, env, **kw):
        r.set_environment(envs[env])
        r.set_option("engine", engine)
        return r.render_into(frame, spp_count=args.spp, **kw)

    forms = [(f, e) for f in ("megakernel", "wavefront") for e in ("none", "sky512")]
    res = {f"{f}/{e}": {q: [] for q in ("wall_ms", "trace_ms", "film_ms", "kernel_ms")} for f, e in forms}
    info = {}
    for f, e in forms:      # warm-up: allocations, code objects
        render(f, e)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for f, e in forms:
            k = f"{f}/{e}"
            r.set_environment(envs[e])      # (the tables are built outside the timed region)
            r.set_option("engine", f)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.render_into(frame, spp_count=args.spp, want_stats=False)
            torch.cuda.synchronize()
            res[k]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            st = r.render_into(frame, spp_count=args.spp, time_kernels=True)
            torch.cuda.synchronize()
            for q in ("trace_ms", "film_ms", "kernel_ms"):
                res[k][q].append(float(st[q]))
            info[k] = {"rays": int(st["n_closest_rays"] + st["n_shadow_rays"]), "engine": int(st["engine"]), "wf_record": st["wf_record"]}
            print(k, it, {q: round(v[-1], 3) for q, v in res[k].items()}, info[k], flush=True)
    summary = {k: {**info[k], **{q: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for q, v in d.items()}}
               for k, d in res.items()}
    for k, s in summary.items():
        s["wall_ns_per_ray"] = s["wall_ms"]["median"] * 1e6 / s["rays"]
    print(json.dumps(summary))
    if args.json:
        json.dump({"spp": args.spp, "set_environment_ms": set_ms, "operators": ops, "runs": res, "summary": summary}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
