"""What the first-hit feature frames cost: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz:
1024 x 1024, the device-built tree) at 16 samples per pixel, alternately in one process and one context,
  normals   nori_hip_render of the same scene with the `normals` integrator: the comparator -- existing code, one closest-hit ray
            and one film pass per camera sample
  one       nori_hip_render_features, one feature (normal)
  three     nori_hip_render_features, albedo + normal + depth: the same trace, two more planes stored, two more film passes
Per run: the wall time of an untimed call and a synchronize, and trace_ms / film_ms / kernel_ms of a second call with
time_kernels on.  Reported as median (min - max) over the runs: the spread is the yardstick for every comparison.
    python tools/features_cost.py [--runs 5] [--spp 16] [--json out.json]"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nori_amd.render import Renderer  # noqa: E402
from nori_amd.scene import Integrator, Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    scn = copy.copy(sc)
    scn.integrator = Integrator("normals")
    r, rn = Renderer(0).upload(sc, builder=2), Renderer(0).upload(scn, builder=2)
    frames = [torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for _ in range(3)]

    def render(form, **kw):
        if form == "normals":
            return rn.render_into(frames[0], spp_count=args.spp, **kw)
        if form == "one":
            return r.render_features_into(normal=frames[1], spp_count=args.spp, **kw)
        return r.render_features_into(albedo=frames[0], normal=frames[1], depth=frames[2], spp_count=args.spp, **kw)

    forms = ["normals", "one", "three"]
    res = {k: {q: [] for q in ("wall_ms", "trace_ms", "film_ms", "kernel_ms")} for k in forms}
    info = {}
    for k in forms:      # warm-up: allocations, code objects
        render(k)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for k in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render(k, want_stats=False)
            torch.cuda.synchronize()
            res[k]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            st = render(k, time_kernels=True)
            torch.cuda.synchronize()
            for q in ("trace_ms", "film_ms", "kernel_ms"):
                res[k][q].append(float(st[q]))
            info[k] = {"rays": int(st["n_closest_rays"] + st["n_shadow_rays"]), "engine": int(st["engine"]), "lds_bytes": int(st["lds_bytes"])}
            print(k, it, {q: round(v[-1], 3) for q, v in res[k].items()}, info[k], flush=True)
    summary = {k: {**info[k], **{q: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for q, v in d.items()}}
               for k, d in res.items()}
    print(json.dumps(summary))
    if args.json:
        json.dump({"spp": args.spp, "runs": res, "summary": summary}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
