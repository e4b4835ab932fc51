"""What the thin lens costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024, the
device-built tree) at 16 samples per pixel, in one process and one context, alternately with the pinhole (radius 0) and with a lens
focused on the back wall (focus distance = the camera-space depth of what the pinhole ray through the frame's centre hits,
radius = 2 % of it),
  megakernel   nori_hip_render, engine = megakernel
  wavefront    nori_hip_render, engine = wavefront
  features     nori_hip_render_features, albedo + normal + depth
Per run: the wall time of an untimed call and a synchronize, and trace_ms / film_ms / kernel_ms of a second call with time_kernels
on.  Reported as median (min - max) over the runs: the spread is the yardstick for every comparison.  A lens render traces other
paths than the pinhole's, so the ray counts are printed beside the times.
    python tools/lens_cost.py [--runs 5] [--spp 16] [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nori_amd import _capi  # noqa: E402
from nori_amd.render import Renderer  # noqa: E402
from nori_amd.scene import Scene  # noqa: E402


def centre_depth(r, sc):
    """camera-space depth t * d.z of the pinhole ray through the middle of the frame (what `nori --focus-pixel` computes)"""
    c = sc.camera
    rays = r.sample_rays(np.array([[c.width // 2 + 0.5, c.height // 2 + 0.5]], np.float32))
    its = r.intersect(rays)
    assert its["mesh"][0] != _capi.NO_HIT, "the centre ray hits nothing"
    axis = np.asarray(c.to_world, np.float64).reshape(4, 4)[:3, 2]
    return float(its["t"][0] * (axis @ rays["d"][0].astype(np.float64)) / (axis @ axis))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    r = Renderer(0).upload(sc, builder=2)
    focus = centre_depth(r, sc)
    lenses = {"pinhole": (0.0, focus), "lens": (0.02 * focus, focus)}
    print("lens:", lenses["lens"], flush=True)
    frames = [torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for _ in range(3)]

    def render(form, lens, **kw):
        r.set_lens(*lenses[lens])
        if form == "features":
            return r.render_features_into(albedo=frames[0], normal=frames[1], depth=frames[2], spp_count=args.spp, **kw)
        r.set_option("engine", form)
        return r.render_into(frames[0], spp_count=args.spp, **kw)

    forms = [(f, l) for f in ("megakernel", "wavefront", "features") for l in ("pinhole", "lens")]
    res = {f"{f}/{l}": {q: [] for q in ("wall_ms", "trace_ms", "film_ms", "kernel_ms")} for f, l in forms}
    info = {}
    for f, l in forms:      # warm-up: allocations, code objects
        render(f, l)
    torch.cuda.synchronize()
    for it in range(args.runs):
        for f, l in forms:
            k = f"{f}/{l}"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render(f, l, want_stats=False)
            torch.cuda.synchronize()
            res[k]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            st = render(f, l, time_kernels=True)
            torch.cuda.synchronize()
            for q in ("trace_ms", "film_ms", "kernel_ms"):
                res[k][q].append(float(st[q]))
            info[k] = {"rays": int(st["n_closest_rays"] + st["n_shadow_rays"]), "engine": int(st["engine"])}
            print(k, it, {q: round(v[-1], 3) for q, v in res[k].items()}, info[k], flush=True)
    summary = {k: {**info[k], **{q: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for q, v in d.items()}}
               for k, d in res.items()}
    print(json.dumps(summary))
    if args.json:
        json.dump({"spp": args.spp, "lens": lenses["lens"], "runs": res, "summary": summary}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
