"""What keeping second moments costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz:
1024 x 1024, 256 spp, path_mis, the device-built tree, wavefront engine) rendered alternately, in one process and one context,
  plain    nori_hip_render
  moments  nori_hip_render_moments: the same samples, every film gather followed by its second pass over the store
Per run: the frame's wall time (an untimed render, then synchronize) and the per-kernel-class times of a second render with
time_kernels on.  The run-to-run spread of `plain` is the yardstick for comparing two builds' plain renders.
    python tools/moments_cost.py [--runs 5] [--json out.json]"""
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
from nori_amd.scene import Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    r = Renderer(0).upload(Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz")), builder=2)
    frame, m2 = (torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for _ in range(2))
    has_moments = hasattr(r, "render_moments_into")      # (the tool also runs on a build without them: `plain` alone)

    def render(form, **kw):
        return r.render_moments_into(frame, m2, **kw) if form == "moments" else r.render_into(frame, **kw)

    forms = ["plain", "moments"] if has_moments else ["plain"]
    res = {k: {q: [] for q in ("frame_ms", "shade_ms", "trace_ms", "film_ms", "kernel_ms")} for k in forms}
    rays = {}
    for k in forms:      # warm-up
        render(k)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for k in forms:
            frame.zero_(); m2.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render(k, want_stats=False)
            torch.cuda.synchronize()
            res[k]["frame_ms"].append((time.perf_counter() - t0) * 1e3)
            frame.zero_(); m2.zero_()
            st = render(k, time_kernels=True)
            torch.cuda.synchronize()
            for q in ("shade_ms", "trace_ms", "film_ms", "kernel_ms"):
                res[k][q].append(float(st[q]))
            rays[k] = int(st["n_closest_rays"] + st["n_shadow_rays"])
            print(k, it, {q: round(v[-1], 2) for q, v in res[k].items()}, "rays", rays[k], flush=True)
    summary = {k: {"rays": rays[k], **{q: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for q, v in d.items()}}
               for k, d in res.items()}
    print(json.dumps(summary))
    if args.json:
        json.dump({"runs": res, "summary": summary}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
