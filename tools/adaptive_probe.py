"""What steering the samples by the tile errors buys: the headline Cornell box
(tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024, path_mis, the device-built tree, engine auto) rendered, per target, by
  adaptive  nori_hip_render_adaptive: passes of --pass-spp samples over the tiles whose error is still above the target
  uniform   nori_hip_render_to_error: the same passes over the whole frame, until the MEAN error of the frame is what the
            adaptive run ended with (the smallest float32 at or above it)
with the same pass_spp and budget (--spp, the most a pixel may get).  Per run: the camera samples spent, the wall time taken around
a synchronise, the final sum_err / n_pixels, and for the adaptive run the histogram of the samples per tile.  Repeats alternate.
    python tools/adaptive_probe.py [--targets 0.08,0.05,0.03] [--pass-spp 16] [--spp 256] [--runs 3] [--json out.json]"""
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
    ap.add_argument("--targets", default="0.08,0.05,0.03")
    ap.add_argument("--pass-spp", type=int, default=16)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    r = Renderer(0).upload(Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz")), builder=2)
    frame, m2 = (torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for _ in range(2))

    def timed(fn):
        frame.zero_(); m2.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    timed(lambda: r.render_moments_into(frame, m2, spp_count=args.pass_spp))      # warm-up: pools, film store
    rows = []
    for target in (float(t) for t in args.targets.split(",")):
        row = {"target_tile_err": target, "pass_spp": args.pass_spp, "budget_spp": args.spp, "adaptive": [], "uniform": []}
        for it in range(args.runs):
            ms, (tile_spp, summary, st) = timed(lambda: r.render_adaptive(frame, m2, target, pass_spp=args.pass_spp, spp_count=args.spp))
            mean = summary["frame"]["sum_err"] / summary["frame"]["n_pixels"]
            values, counts = np.unique(tile_spp.cpu().numpy(), return_counts=True)
            row["adaptive"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "mean_err": mean, "max_err": summary["frame"]["max_err"],
                                    "passes": summary["passes"], "n_unconverged": summary["n_unconverged"],
                                    "tile_spp_histogram": {int(v): int(c) for v, c in zip(values, counts)}})
            goal = np.float32(mean)
            if float(goal) < mean:
                goal = np.nextafter(goal, np.float32(np.inf))
            ms, (done, last, st) = timed(lambda: r.render_to_error(frame, m2, float(goal), pass_spp=args.pass_spp, spp_count=args.spp))
            row["uniform"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "mean_err": last["sum_err"] / last["n_pixels"],
                                   "max_err": last["max_err"], "spp_done": done})
            print(json.dumps({"target": target, "run": it, "adaptive": row["adaptive"][-1], "uniform": row["uniform"][-1]}), flush=True)
        for form in ("adaptive", "uniform"):
            ms = [x["ms"] for x in row[form]]
            row[form + "_ms"] = {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}
        rows.append(row)
    print(json.dumps({"summary": [{k: v for k, v in row.items() if k not in ("adaptive", "uniform")} | {"adaptive_samples": row["adaptive"][0]["camera_samples"],
                                   "uniform_samples": row["uniform"][0]["camera_samples"], "adaptive_mean_err": row["adaptive"][0]["mean_err"],
                                   "uniform_mean_err": row["uniform"][0]["mean_err"]} for row in rows]}))
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
