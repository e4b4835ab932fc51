"""What a delta light costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024, the
device-built tree) at 16 samples per pixel, in one process and one context, alternately without lights and with ONE point light
in the middle of the box, on both engines.  With the light the context leaves the all-diffuse kernels and the compact path record
for the general variant (MATSET 159, the full record), and half of its emitter samples go to the point light, whose shadow rays
end elsewhere -- so the ray counts are printed beside the times.
Per run: the wall time of an untimed call and a synchronize, and trace_ms / film_ms / kernel_ms of a second call with time_kernels
on.  Reported as median (min - max) over the runs: the spread is the yardstick for every comparison.
    python tools/lights_cost.py [--runs 5] [--spp 16] [--json profiles/lights_cost.json]"""
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
from nori_amd.scene import Light, Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    pts = np.concatenate([m.positions for m in sc.meshes])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    extent = float((hi - lo).max())
    light = Light("point", tuple(float(x) for x in (lo + hi) / 2), intensity=(extent * extent,) * 3)
    sets = {"none": [], "point": [light]}
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")

    forms = [(f, e) for f in ("megakernel", "wavefront") for e in ("none", "point")]
    res = {f"{f}/{e}": {q: [] for q in ("wall_ms", "trace_ms", "film_ms", "kernel_ms")} for f, e in forms}
    info = {}
    for f, e in forms:      # warm-up: allocations, code objects
        r.set_lights(sets[e])
        r.set_option("engine", f)
        r.render_into(frame, spp_count=args.spp)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for f, e in forms:
            k = f"{f}/{e}"
            r.set_lights(sets[e])
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
            info[k] = {"closest_rays": int(st["n_closest_rays"]), "shadow_rays": int(st["n_shadow_rays"]), "rays": int(st["n_closest_rays"] + st["n_shadow_rays"]),
                       "engine": int(st["engine"]), "wf_record": st["wf_record"]}
            print(k, it, {q: round(v[-1], 3) for q, v in res[k].items()}, info[k], flush=True)
    summary = {k: {**info[k], **{q: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for q, v in d.items()}}
               for k, d in res.items()}
    for k, s in summary.items():
        s["wall_ns_per_ray"] = s["wall_ms"]["median"] * 1e6 / s["rays"]
    print(json.dumps(summary))
    if args.json:
        json.dump({"spp": args.spp, "light": {"type": "point", "position": list(light.position), "intensity": list(light.intensity)}, "runs": res, "summary": summary},
                  open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
