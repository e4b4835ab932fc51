"""What planning the samples from a pilot buys: the headline Cornell box
(tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024, path_mis, the device-built tree, engine auto), budget --spp, per target three arms:
  old      the existing loop: nori_hip_render_adaptive (raw targets) / nori_hip_render_adaptive_denoised (denoised targets), --pass-spp
  new      nori_hip_render_allocated, metric 0 / 1: a pilot of --pilot-spp, at most --rounds rounds, --headroom
  uniform  raw: nori_hip_render_to_error in passes of --pass-spp until the MEAN error of the frame is what the new arm ended with (the
           smallest float32 at or above it), as tools/adaptive_probe.py does.  Denoised: nori_hip_render_moments of N spp and
           nori_hip_denoise_var, N = the smallest multiple of --pass-spp whose predicted mean error of the denoised frame is at or below
           the new arm's (found beforehand, untimed, by adding passes to one pair of frames).
The arms alternate in one process, --runs repeats; wall ms around a synchronise.  Per run: camera samples, render calls, the final mean and
maximum error (of the arm's metric), tiles above the target, the tile_spp histogram; for the denoised arms also the TRUE trimmed relative
squared error (tests/denoise_ref.trimmed_error) against --ref-spp samples of a disjoint range.  The feature frames (--feature-spp) are
rendered once and serve all arms.
    python tools/allocate_probe.py [--raw-targets 0.08,0.05,0.03] [--denoised-targets 0.01082,0.00596,0.00442] [--runs 3] [--json out.json]"""
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
from tests.denoise_ref import trimmed_error  # noqa: E402

NAMES = ("albedo", "normal", "depth")


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def histogram(tile_spp):
    values, counts = np.unique(tile_spp.cpu().numpy(), return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw-targets", default="0.08,0.05,0.03")
    ap.add_argument("--denoised-targets", default="0.01082,0.00596,0.00442")
    ap.add_argument("--pass-spp", type=int, default=16)
    ap.add_argument("--pilot-spp", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--headroom", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--feature-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    c = sc.camera
    K, N = args.pass_spp, args.spp
    alloc = dict(pilot_spp=args.pilot_spp, max_rounds=args.rounds, headroom=args.headroom, spp_count=N)
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    frame, m2 = zeros(), zeros()
    feats = {k: zeros() for k in NAMES}
    rgb, var = (torch.zeros((c.height, c.width, 3), device="cuda:0") for _ in range(2))
    wsum = torch.zeros((c.height, c.width), device="cuda:0")

    def timed(fn):
        frame.zero_(); m2.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def mean_of(frame_summary):
        return frame_summary["sum_err"] / frame_summary["n_pixels"]

    r.render_features_into(**feats, spp_count=args.feature_spp, want_stats=False)
    timed(lambda: r.render_moments_into(frame, m2, spp_count=K))      # warm-up: pools, film store
    timed(lambda: r.render_allocated(frame, m2, 0.05, **alloc))       # ... and the lists
    timed(lambda: r.render_allocated(frame, m2, 0.005, **feats, metric=1, **alloc))

    rows = []
    # ---- the raw metric
    for target in (float(t) for t in args.raw_targets.split(",") if t):
        row = {"metric": "raw", "target_tile_err": target, "budget_spp": N, "old": [], "new": [], "uniform": []}
        for it in range(args.runs):
            ms, (tile_spp, summary, st) = timed(lambda: r.render_adaptive(frame, m2, target, pass_spp=K, spp_count=N))
            row["old"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "render_calls": summary["passes"], "mean_err": mean_of(summary["frame"]),
                               "max_err": summary["frame"]["max_err"], "n_unconverged": summary["n_unconverged"], "tile_spp_histogram": histogram(tile_spp)})
            ms, (tile_spp, log, summary, st) = timed(lambda: r.render_allocated(frame, m2, target, **alloc))
            mean = mean_of(summary["frame"])
            row["new"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "render_calls": summary["passes"], "mean_err": mean,
                               "max_err": summary["frame"]["max_err"], "n_unconverged": summary["n_unconverged"], "tile_spp_histogram": histogram(tile_spp)})
            goal = np.float32(mean)
            if float(goal) < mean:
                goal = np.nextafter(goal, np.float32(np.inf))
            ms, (done, last, st) = timed(lambda: r.render_to_error(frame, m2, float(goal), pass_spp=K, spp_count=N))
            row["uniform"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "render_calls": (done + K - 1) // K, "mean_err": mean_of(last),
                                   "max_err": last["max_err"], "spp_done": done})
            print(json.dumps({"metric": "raw", "target": target, "run": it, **{arm: row[arm][-1] for arm in ("old", "new", "uniform")}}), flush=True)
        rows.append(row)

    # ---- the denoised metric: the reference, and uniform frames pass by pass (the predicted and the true error of every multiple of K)
    denoised_targets = [float(t) for t in args.denoised_targets.split(",") if t]
    uniform = {}
    if denoised_targets:
        ref = zeros()
        for begin in range(100000, 100000 + args.ref_spp, 1024):
            r.render_into(ref, spp_count=min(1024, 100000 + args.ref_spp - begin), spp_begin=begin, want_stats=False)
        torch.cuda.synchronize()
        b = r.border
        core = ref[b:ref.shape[0] - b, b:ref.shape[1] - b]
        ref = (core[..., :3] / core[..., 3:4]).cpu().numpy()

        def quality(out_rgb, out_var, out_wsum):
            _, s = r.denoised_error_map(out_rgb, out_var, out_wsum, want_map=False)
            return {"mean_err": mean_of(s), "max_err": s["max_err"], "true_trimmed_err": trimmed_error(out_rgb.cpu().numpy(), ref)}

        frame.zero_(); m2.zero_()
        for k in range((N + K - 1) // K):
            r.render_moments_into(frame, m2, spp_count=min(K, N - k * K), spp_begin=k * K, want_stats=False)
            r.denoise_var_into(rgb, var, frame, m2, wsum=wsum, **feats)
            uniform[min(N, (k + 1) * K)] = quality(rgb, var, wsum)
    for target in denoised_targets:
        row = {"metric": "denoised", "target_tile_err": target, "budget_spp": N, "old": [], "new": [], "uniform": []}
        n_uniform = None
        for it in range(args.runs):
            ms, (o_rgb, o_var, o_wsum, tile_spp, summary, st) = timed(lambda: r.render_adaptive_denoised(frame, m2, target, **feats, pass_spp=K, spp_count=N))
            row["old"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "render_calls": summary["passes"], "n_unconverged": summary["n_unconverged"],
                               "tile_spp_histogram": histogram(tile_spp), **quality(o_rgb, o_var, o_wsum)})
            ms, (o_rgb, o_var, o_wsum, tile_spp, log, summary, st) = timed(lambda: r.render_allocated(frame, m2, target, **feats, metric=1, **alloc))
            row["new"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "render_calls": summary["passes"], "n_unconverged": summary["n_unconverged"],
                               "tile_spp_histogram": histogram(tile_spp), **quality(o_rgb, o_var, o_wsum)})
            if n_uniform is None:
                ok = [spp for spp, q in sorted(uniform.items()) if q["mean_err"] <= row["new"][-1]["mean_err"]]
                n_uniform = ok[0] if ok else N
                row["uniform_spp"] = n_uniform

            def arm3():
                st = r.render_moments_into(frame, m2, spp_count=n_uniform)
                r.denoise_var_into(rgb, var, frame, m2, wsum=wsum, **feats)
                return st
            ms, st = timed(arm3)
            row["uniform"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "render_calls": 1, "spp_done": n_uniform, **uniform[n_uniform]})
            print(json.dumps({"metric": "denoised", "target": target, "run": it, **{arm: row[arm][-1] for arm in ("old", "new", "uniform")}}), flush=True)
        rows.append(row)

    for row in rows:
        for arm in ("old", "new", "uniform"):
            row[arm + "_ms"] = stat([x["ms"] for x in row[arm]])
        print(json.dumps({k: v for k, v in row.items() if k not in ("old", "new", "uniform")} | {arm + "_first": row[arm][0] for arm in ("old", "new", "uniform")}), flush=True)
    out = {"scene": "pa4-cbox-path_mis 1024 x 1024", "filter": sc.rfilter.type, "pass_spp": K, "pilot_spp": args.pilot_spp, "max_rounds": args.rounds, "headroom": args.headroom,
           "budget_spp": N, "feature_spp": args.feature_spp, "reference_spp": args.ref_spp, "reference_spp_begin": 100000, "runs": args.runs,
           "uniform_denoised_by_spp": {str(k): v for k, v in uniform.items()}, "rows": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(out, open(args.json, "w"), indent=1)
    r.close()


if __name__ == "__main__":
    main()
