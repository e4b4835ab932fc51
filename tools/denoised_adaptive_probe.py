"""What stopping on the error of the DENOISED frame buys: the headline Cornell box
(tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024, path_mis, the device-built tree, engine auto), per target three arms:
  1 denoised-adaptive  nori_hip_render_adaptive_denoised: tiles retire on the denoised tile errors
  2 adaptive+denoise   nori_hip_render_adaptive to the same target (raw tile errors), then nori_hip_denoise
  3 uniform+denoise    nori_hip_render_moments of N spp, then nori_hip_denoise; N = the smallest multiple of --pass-spp whose TRUE error
                       is at or below arm 1's (found beforehand, untimed, by adding passes to one pair of frames)
with the same pass_spp and budget (--spp, the most a pixel may get).  The feature frames (--feature-spp) are rendered once and
serve all arms; their time is reported beside the arms, not inside them.  Per arm: camera samples, wall ms around a synchronise as
median (min - max) over alternating repeats in one process, passes, the tile_spp histogram, the predicted mean error (the mean of
nori_hip_denoised_error_map), the TRUE trimmed relative squared error (tests/denoise_ref.trimmed_error) against --ref-spp samples of a
disjoint range, and mean squared error / mean predicted variance.  --filter box replaces the scene's reconstruction filter.
--targets auto takes the 75th, 50th and 25th percentile of the non-zero denoised tile errors at 2 x pass_spp (recorded in the output).
  --cost: the variance filter against nori_hip_denoise at the defaults and at R = 8, F = 2, alternating, event ms on 16-spp frames.
    python tools/denoised_adaptive_probe.py [--targets auto|a,b,c] [--pass-spp 16] [--spp 256] [--runs 3] [--filter scene|box] [--json out.json]
    python tools/denoised_adaptive_probe.py --cost [--runs 7] [--json out.json]"""
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
from nori_amd.scene import RFilter, Scene  # noqa: E402
from tests.denoise_ref import trimmed_error  # noqa: E402

NAMES = ("albedo", "normal", "depth")


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def develop(r, rgbw):
    b = r.border
    c = rgbw[b:rgbw.shape[0] - b, b:rgbw.shape[1] - b]
    return (c[..., :3] / c[..., 3:4]).cpu().numpy()


def histogram(tile_spp):
    values, counts = np.unique(tile_spp.cpu().numpy(), return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


def cost(r, runs):
    c = r.scene.camera
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    f = {k: zeros() for k in ("rgbw", "m2") + NAMES}
    r.render_moments_into(f["rgbw"], f["m2"], spp_count=16, want_stats=False)
    r.render_features_into(**{k: f[k] for k in NAMES}, spp_count=16, want_stats=False)
    feats = {k: f[k] for k in NAMES}
    rgb, var = (torch.zeros((c.height, c.width, 3), device="cuda:0") for _ in range(2))
    wsum = torch.zeros((c.height, c.width), device="cuda:0")
    forms = {}
    for name, params in (("R5 F1", {}), ("R8 F2", dict(radius=8, patch=2))):
        forms["denoise " + name] = lambda params=params: r.denoise_into(rgb, f["rgbw"], f["m2"], wsum=wsum, **feats, **params)
        forms["denoise_var " + name] = lambda params=params: r.denoise_var_into(rgb, var, f["rgbw"], f["m2"], wsum=wsum, **feats, **params)
    res = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for it in range(runs):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b))
        print(it, {k: round(v[-1], 3) for k, v in res.items()}, flush=True)
    out = {"spp": 16, "width": c.width, "height": c.height, "event_ms (steps A + B)": {k: stat(v) for k, v in res.items()}, "runs": res}
    for name in ("R5 F1", "R8 F2"):
        out["ratio " + name] = float(np.median(res["denoise_var " + name]) / np.median(res["denoise " + name]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="auto")
    ap.add_argument("--pass-spp", type=int, default=16)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--feature-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--filter", default="scene", choices=("scene", "box"))
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    if args.filter == "box":
        sc = copy.copy(sc)
        sc.rfilter = RFilter("box")
    r = Renderer(0).upload(sc, builder=2)
    if args.cost:
        out = cost(r, args.runs)
        print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
        if args.json:
            json.dump(out, open(args.json, "w"), indent=1)
        return
    c = sc.camera
    K, N = args.pass_spp, args.spp
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

    feature_ms = []
    for it in range(3):      # (the first is the warm-up)
        for t in feats.values():
            t.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.render_features_into(**feats, spp_count=args.feature_spp, want_stats=False)
        torch.cuda.synchronize()
        feature_ms.append((time.perf_counter() - t0) * 1e3)
    timed(lambda: r.render_moments_into(frame, m2, spp_count=K))      # warm-up: pools, film store

    ref = zeros()
    for begin in range(100000, 100000 + args.ref_spp, 1024):
        r.render_into(ref, spp_count=min(1024, 100000 + args.ref_spp - begin), spp_begin=begin, want_stats=False)
    torch.cuda.synchronize()
    ref = develop(r, ref)
    ref64 = ref.astype(np.float64)

    def measure(x, y):
        """of the frames as they stand: predicted mean error, true trimmed error, mse / mean predicted variance (denoise_var: nori_hip_denoise's bits)"""
        r.denoise_var_into(rgb, var, x, y, wsum=wsum, **feats)
        _, s = r.denoised_error_map(rgb, var, wsum, want_map=False)
        out, v = rgb.cpu().numpy(), var.cpu().numpy().astype(np.float64)
        mse = float(((out.astype(np.float64) - ref64) ** 2).mean())
        return {"predicted_mean_err": s["sum_err"] / s["n_pixels"], "true_trimmed_err": trimmed_error(out, ref), "mse": mse, "mse_over_predicted_variance": mse / float(v.mean())}

    # uniform frames pass by pass, once: the true error of a uniform render of every multiple of K, and the targets
    frame.zero_(); m2.zero_()
    uniform = {}
    auto = None
    for k in range((N + K - 1) // K):
        r.render_moments_into(frame, m2, spp_count=min(K, N - k * K), spp_begin=k * K, want_stats=False)
        spp = min(N, (k + 1) * K)
        uniform[spp] = measure(frame, m2)
        print("uniform", spp, uniform[spp], flush=True)
        if spp == 2 * K:
            te = np.sort(r.denoised_tile_errors(rgb, var, wsum).cpu().numpy().reshape(-1))
            lit = te[te > 0]      # (tiles that see nothing but the background have error 0 and retire at the first evaluation whatever the target)
            auto = [float(np.float32(lit[int(q * (lit.size - 1))])) for q in (0.75, 0.5, 0.25)]
            print("denoised tile errors at", spp, "spp:", te.size - lit.size, "tiles of error 0; of the others min", lit[0], "quartiles", auto[::-1], "max", lit[-1], flush=True)
    targets = auto if args.targets == "auto" else [float(t) for t in args.targets.split(",")]

    rows = []
    for target in targets:
        row = {"target_tile_err": target, "pass_spp": K, "budget_spp": N, "arm1": [], "arm2": [], "arm3": []}
        n_uniform = None
        for it in range(args.runs):
            ms, (_, _, _, tile_spp, summary, st) = timed(lambda: r.render_adaptive_denoised(frame, m2, target, **feats, pass_spp=K, spp_count=N))
            a1 = {"ms": ms, "camera_samples": int(st["n_camera_samples"]), "passes": summary["passes"], "n_unconverged": summary["n_unconverged"],
                  "tile_spp_histogram": histogram(tile_spp)}
            if it == 0:
                row["arm1_quality"] = measure(frame, m2)
                ok = [spp for spp, q in sorted(uniform.items()) if q["true_trimmed_err"] <= row["arm1_quality"]["true_trimmed_err"]]
                n_uniform = ok[0] if ok else None
                row["arm3_spp"] = n_uniform
            row["arm1"].append(a1)

            def arm2():
                out = r.render_adaptive(frame, m2, target, pass_spp=K, spp_count=N)
                r.denoise_into(rgb, frame, m2, wsum=wsum, **feats)
                return out
            ms, (tile_spp, summary, st) = timed(arm2)
            row["arm2"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "passes": summary["passes"], "n_unconverged": summary["n_unconverged"],
                                "tile_spp_histogram": histogram(tile_spp)})
            if it == 0:
                row["arm2_quality"] = measure(frame, m2)
            if n_uniform is not None:
                def arm3():
                    st = r.render_moments_into(frame, m2, spp_count=n_uniform)
                    r.denoise_into(rgb, frame, m2, wsum=wsum, **feats)
                    return st
                ms, st = timed(arm3)
                row["arm3"].append({"ms": ms, "camera_samples": int(st["n_camera_samples"]), "spp": n_uniform})
                if it == 0:
                    row["arm3_quality"] = uniform[n_uniform]
            print(json.dumps({"target": target, "run": it, "arm1": row["arm1"][-1], "arm2": row["arm2"][-1], "arm3": row["arm3"][-1] if row["arm3"] else None}), flush=True)
        for arm in ("arm1", "arm2", "arm3"):
            if row[arm]:
                row[arm + "_ms"] = stat([x["ms"] for x in row[arm]])
        print(json.dumps({k: v for k, v in row.items() if k not in ("arm1", "arm2", "arm3")}), flush=True)
        rows.append(row)
    out = {"scene": "pa4-cbox-path_mis 1024 x 1024", "filter": sc.rfilter.type, "feature_spp": args.feature_spp, "feature_ms": feature_ms, "reference_spp": args.ref_spp,
           "reference_spp_begin": 100000, "targets": targets, "targets_chosen": args.targets, "uniform": {str(k): v for k, v in uniform.items()}, "rows": rows}
    if args.json:
        json.dump(out, open(args.json, "w"), indent=1)
    r.close()


if __name__ == "__main__":
    main()
