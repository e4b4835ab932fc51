"""What a grid medium costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024, the
device-built tree) at 16 samples per pixel, in one process and one context, alternating between fills that enclose the box and the
camera: the homogeneous medium whose mean free path is the box's size, and a 1^3, a 32^3 and a 128^3 grid of the same constant
density -- the same medium, so the paths are the same up to where a free flight leaves the grid's box, and what differs is the walk:
1, about 32 and about 128 voxels per query.  Both engines.  Per run: the wall time of an untimed call and a synchronize, and
trace_ms / film_ms / kernel_ms of a second call with time_kernels on.  Reported as median (min - max) over the runs: the spread is
the yardstick for every comparison.  Also reported: the voxels a camera ray visits in each grid (nori_hip_grid_medium_optical_depth
on the centres of 4096 pixels).
    python tools/grid_medium_cost.py [--runs 5] [--spp 16] [--json profiles/grid_medium_cost.json]"""
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
from nori_amd.scene import GridMedium, Medium, Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    pts = np.concatenate([m.positions for m in sc.meshes] + [np.asarray(sc.camera.to_world, np.float64)[:3, 3][None, :]])
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    extent = float((hi - lo).max())
    sigma, albedo, g = 1.0 / extent, (0.9, 0.8, 0.7), 0.6
    bmin, bmax = tuple(lo - 0.05 * extent), tuple(hi + 0.05 * extent)
    fills = {"homogeneous": Medium(sigma, albedo, g)}
    for n in (1, 32, 128):
        fills[f"grid_{n}"] = GridMedium(np.ones((n, n, n), np.float32), bmin, bmax, sigma, albedo, g)
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")

    # the voxels a camera ray visits
    w, h = sc.camera.width, sc.camera.height
    px = np.stack(np.meshgrid(np.arange(8, w, 16), np.arange(8, h, 16)), -1).reshape(-1, 2).astype(np.float32) + 0.5
    rays = r.sample_rays(px)
    voxels = {}
    for name, m in fills.items():
        if name == "homogeneous":
            continue
        r.set_medium(m)
        tau, steps = r.grid_medium_optical_depth(rays["o"], rays["d"], np.full(px.shape[0], np.inf, np.float32))
        voxels[name] = {"queries": int(px.shape[0]), "mean": float(steps.mean()), "min": int(steps.min()), "max": int(steps.max()), "mean_tau": float(tau.mean())}
        print(name, "voxels per camera ray", voxels[name], flush=True)

    forms = [(f, e) for f in ("megakernel", "wavefront") for e in fills]
    res = {f"{f}/{e}": {q: [] for q in ("wall_ms", "trace_ms", "film_ms", "kernel_ms")} for f, e in forms}
    info = {}
    for f, e in forms:      # warm-up: allocations, code objects
        r.set_medium(fills[e])
        r.set_option("engine", f)
        r.render_into(frame, spp_count=args.spp)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for f, e in forms:
            k = f"{f}/{e}"
            r.set_medium(fills[e])
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
            info[k] = {"rays": int(st["n_closest_rays"] + st["n_shadow_rays"]), "engine": int(st["engine"])}
            print(k, it, {q: round(v[-1], 3) for q, v in res[k].items()}, info[k], flush=True)
    summary = {k: {**info[k], **{q: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for q, v in d.items()}}
               for k, d in res.items()}
    for k, s in summary.items():
        s["wall_ns_per_ray"] = s["wall_ms"]["median"] * 1e6 / s["rays"]
        print(k, "wall %.2f (%.2f - %.2f) ms, %d rays, %.3f ns per ray" % (s["wall_ms"]["median"], s["wall_ms"]["min"], s["wall_ms"]["max"], s["rays"], s["wall_ns_per_ray"]))
    if args.json:
        json.dump({"spp": args.spp, "medium": {"sigma": sigma, "albedo": list(albedo), "g": g, "bmin": list(bmin), "bmax": list(bmax)},
                   "voxels_per_camera_ray": voxels, "runs": res, "summary": summary}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
