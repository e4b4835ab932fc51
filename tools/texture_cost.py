"""What a textured hit costs: the headline Cornell box (tests/golden/pa4-cbox-path_mis.npz: 1024 x 1024,
256 spp, path_mis, the device-built tree, wavefront engine) rendered alternately in three forms, in one process:
  plain           the scene as it is
  textured_const  walls, floor and ceiling (meshes 0, 1, 2) each with a 1024 x 1024 bilinear, repeat image at uv scale 4 whose
                  texels all equal the mesh's albedo: the same paths and ray counts as `plain`, only the texture reads added
  textured        the same images with texels = albedo x U(0.5, 1) (seed 0): a darker scene, shorter paths
Per run: the frame's wall time (an untimed render, then synchronize) and the per-kernel-class times of a second render with
time_kernels on.
    python tools/texture_cost.py [--runs 5] [--json out.json]"""
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
from nori_amd.scene import Scene, Texture  # noqa: E402


def scenes():
    path = os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz")
    out = {"plain": Scene.load_npz(path)}
    rng = np.random.default_rng(0)
    for name in ("textured_const", "textured"):
        sc = Scene.load_npz(path)
        for k, mi in enumerate((0, 1, 2)):
            albedo = np.float32(sc.meshes[mi].bsdf.albedo)
            img = np.broadcast_to(albedo, (1024, 1024, 3)) if name == "textured_const" else albedo * rng.uniform(0.5, 1.0, (1024, 1024, 1))
            sc.textures.append(Texture("image", np.ascontiguousarray(img, np.float32), "bilinear", "repeat", 4.0, 4.0))
            sc.meshes[mi].albedo_texture = k
        out[name] = sc
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rs = {k: Renderer(0).upload(sc, builder=2) for k, sc in scenes().items()}
    frames = {k: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for k, r in rs.items()}
    res = {k: {q: [] for q in ("frame_ms", "shade_ms", "trace_ms", "film_ms", "kernel_ms")} for k in rs}
    rays = {}
    for k, r in rs.items():      # warm-up
        r.render_into(frames[k])
    torch.cuda.synchronize()
    for it in range(args.runs):
        for k, r in rs.items():
            frames[k].zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.render_into(frames[k], want_stats=False)
            torch.cuda.synchronize()
            res[k]["frame_ms"].append((time.perf_counter() - t0) * 1e3)
            frames[k].zero_()
            st = r.render_into(frames[k], time_kernels=True)
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
