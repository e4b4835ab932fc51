"""What the denoiser costs and what it buys: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz:
1024 x 1024, the device-built tree).
  cost     at 16 and at 64 spp, alternately in one process and one context: the render through nori_hip_render_moments, the three feature frames,
           step A alone (nori_hip_denoise_guides) and steps A + B (nori_hip_denoise) on the rendered frames -- wall time of a call
           and a synchronize, and the time between two events on the stream; the filter's own time is (A + B) - A of the same run.
           At 16 spp the same for variants of the window, the patch and the feature terms: the experiment that shows what the filter's
           time follows (taps, patch reads, the divisions of the feature terms).
  quality  at 16 and 64 spp, under the scene's own reconstruction filter and under the box filter: the trimmed relative squared error
           (tests/denoise_ref.py: trimmed_error) of the noisy and of the denoised frame against a render of 8192 spp from a disjoint
           sample range, and their ratio.
Reported as median (min - max) over the runs: the spread is the yardstick for every comparison.
    python tools/denoise_probe.py [--runs 5] [--cost-json profiles/denoise_cost.json] [--quality-json profiles/denoise_quality.json]"""
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

VARIANTS = {      # name: (feature terms, parameters)
    "default R5 F1": (("albedo", "normal", "depth"), {}),
    "no features": ((), {}),
    "R5 F0": (("albedo", "normal", "depth"), dict(patch=0)),
    "R5 F2": (("albedo", "normal", "depth"), dict(patch=2)),
    "R3 F1": (("albedo", "normal", "depth"), dict(radius=3)),
    "R8 F1": (("albedo", "normal", "depth"), dict(radius=8)),
    "R8 F2": (("albedo", "normal", "depth"), dict(radius=8, patch=2)),
}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn):
    """(wall ms of call + synchronize, ms between two events around the call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def frames_of(r, spp):
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    f = {k: zeros() for k in ("rgbw", "m2", "albedo", "normal", "depth")}
    r.render_moments_into(f["rgbw"], f["m2"], spp_count=spp, want_stats=False)
    r.render_features_into(albedo=f["albedo"], normal=f["normal"], depth=f["depth"], spp_count=spp, want_stats=False)
    torch.cuda.synchronize()
    return f


def develop(r, rgbw):
    b = r.border
    c = rgbw[b:rgbw.shape[0] - b, b:rgbw.shape[1] - b]
    return (c[..., :3] / c[..., 3:4]).cpu().numpy()


def cost(r, runs, spp, variants):
    c = r.scene.camera
    f = frames_of(r, spp)
    out, wsum = torch.zeros((c.height, c.width, 3), device="cuda:0"), torch.zeros((c.height, c.width), device="cuda:0")
    guides = torch.zeros((c.height, c.width, 16), device="cuda:0")
    scratch = {k: torch.zeros_like(v) for k, v in f.items()}
    feats = {k: f[k] for k in ("albedo", "normal", "depth")}
    forms = {
        "render_moments": lambda: r.render_moments_into(scratch["rgbw"], scratch["m2"], spp_count=spp, want_stats=False),
        "render_features": lambda: r.render_features_into(albedo=scratch["albedo"], normal=scratch["normal"], depth=scratch["depth"], spp_count=spp, want_stats=False),
        "guides": lambda: r.denoise_guides_into(guides, f["rgbw"], f["m2"], **feats),
    }
    for name, (terms, params) in variants.items():
        forms["denoise " + name] = (lambda terms=terms, params=params: r.denoise_into(out, f["rgbw"], f["m2"], wsum=wsum, **{k: feats[k] for k in terms}, **params))
    res = {k: {"wall_ms": [], "event_ms": []} for k in forms}
    for fn in forms.values():      # warm-up: allocations, code objects
        fn()
    torch.cuda.synchronize()
    for it in range(runs):
        for k, fn in forms.items():
            w, e = timed(fn)
            res[k]["wall_ms"].append(w); res[k]["event_ms"].append(e)
        print(it, {k: round(v["event_ms"][-1], 3) for k, v in res.items()}, flush=True)
    summary = {k: {q: stat(v) for q, v in d.items()} for k, d in res.items()}
    for name, (terms, params) in variants.items():
        filt = [a - g for a, g in zip(res["denoise " + name]["event_ms"], res["guides"]["event_ms"])]
        R = params.get("radius", 5)
        summary["denoise " + name]["filter_ms"] = stat(filt)
        summary["denoise " + name]["filter_ns_per_pixel_tap"] = float(np.median(filt)) * 1e6 / (c.width * c.height * (2 * R + 1) ** 2)
    return {"spp": spp, "width": c.width, "height": c.height, "runs": res, "summary": summary}


def quality(sc, label):
    r = Renderer(0).upload(sc, builder=2)
    ref = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    for begin in range(100000, 100000 + 8192, 1024):
        r.render_into(ref, spp_count=1024, spp_begin=begin, want_stats=False)
    torch.cuda.synchronize()
    ref = develop(r, ref)
    c = sc.camera
    out, wsum = torch.zeros((c.height, c.width, 3), device="cuda:0"), torch.zeros((c.height, c.width), device="cuda:0")
    rows = {}
    for spp in (16, 64):
        f = frames_of(r, spp)
        r.denoise_into(out, f["rgbw"], f["m2"], albedo=f["albedo"], normal=f["normal"], depth=f["depth"], wsum=wsum)
        torch.cuda.synchronize()
        e_noisy, e_den = trimmed_error(develop(r, f["rgbw"]), ref), trimmed_error(out.cpu().numpy(), ref)
        rows[str(spp)] = {"noisy": e_noisy, "denoised": e_den, "ratio": e_den / e_noisy, "wsum_min": float(wsum.min()), "wsum_mean": float(wsum.mean())}
        print(label, spp, rows[str(spp)], flush=True)
    r.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cost-json", default=None)
    ap.add_argument("--quality-json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    costs = {"16": cost(r, args.runs, 16, VARIANTS), "64": cost(r, args.runs, 64, {"default R5 F1": VARIANTS["default R5 F1"]})}
    r.close()
    print(json.dumps({k: v["summary"] for k, v in costs.items()}))
    if args.cost_json:
        json.dump(costs, open(args.cost_json, "w"), indent=1)
    box = copy.copy(sc)
    box.rfilter = RFilter("box")
    q = {"reference_spp": 8192, "reference_spp_begin": 100000, "metric": "mean over the pixels but the worst 1 % of sum_c (x - ref)^2 / (sum_c ref^2 + 0.01)",
         "scene filter (" + sc.rfilter.type + ")": quality(sc, "scene filter"), "box filter": quality(box, "box filter")}
    print(json.dumps(q))
    if args.quality_json:
        json.dump(q, open(args.quality_json, "w"), indent=1)


if __name__ == "__main__":
    main()
