"""What a homogeneous medium costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024,
the device-built tree) at 16 samples per pixel, in one process and one context, alternately without a medium and in a fog whose mean
free path is the box's size (albedo 0.9 / 0.8 / 0.7, g = 0.6), on both engines.  In fog the render traces OTHER paths -- a vertex
every free flight, none of them ends by leaving the box --, so the ray counts are printed beside the times, and the comparison that
isolates the kernels' own cost is time per ray.  Also timed: the operator twins on 2^20 samples.
Per run: the wall time of an untimed call and a synchronize, and trace_ms / film_ms / kernel_ms of a second call with time_kernels
on.  Reported as median (min - max) over the runs: the spread is the yardstick for every comparison.
    python tools/medium_cost.py [--runs 5] [--spp 16] [--json profiles/medium_cost.json]"""
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
from nori_amd.scene import Medium, Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    pts = np.concatenate([m.positions for m in sc.meshes])
    extent = float((pts.max(axis=0) - pts.min(axis=0)).max())
    media = {"none": None, "fog": Medium(1.0 / extent, (0.9, 0.8, 0.7), 0.6)}
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")

    r.set_medium(media["fog"])
    rng = np.random.default_rng(0)
    xi = rng.random((1 << 20, 2), dtype=np.float32)
    d = rng.normal(size=(1 << 20, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ops = {}
    for name, call in (("medium_distance", lambda: r.medium_distance(xi[:, 0])), ("medium_transmittance", lambda: r.medium_transmittance(xi[:, 1] * 10)),
                       ("phase_sample", lambda: r.phase_sample(d, xi)), ("phase_eval", lambda: r.phase_eval(d, d[::-1].copy()))):
        call()      # warm-up: code objects
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        ops[name] = {"n": 1 << 20, "wall_ms_with_copies": float(np.median(ts))}
        print(name, ops[name], flush=True)

    def render(engine, env, **kw):
        r.set_medium(media[env])
        r.set_option("engine", engine)
        return r.render_into(frame, spp_count=args.spp, **kw)

    forms = [(f, e) for f in ("megakernel", "wavefront") for e in ("none", "fog")]
    res = {f"{f}/{e}": {q: [] for q in ("wall_ms", "trace_ms", "film_ms", "kernel_ms")} for f, e in forms}
    info = {}
    for f, e in forms:      # warm-up: allocations, code objects
        render(f, e)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for f, e in forms:
            k = f"{f}/{e}"
            r.set_medium(media[e])
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
        json.dump({"spp": args.spp, "medium": {"sigma_t": 1.0 / extent, "albedo": [0.9, 0.8, 0.7], "g": 0.6}, "operators": ops, "runs": res, "summary": summary}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
