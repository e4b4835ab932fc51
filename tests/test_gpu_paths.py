"""path_mats / path_ems / path_mis with a fog or a sky on EVERY material, bit for bit against tests/path_ref.py: the general kernels
of the kEnvLit / kMedium variants (rt_path.h: path_on_closest, sample_direct) as li_kernel, the megakernel and the wavefront engine
instantiate them, wf_shade's LDSTAB = false readers included -- on scenes with mirror, glass, microfacet and textured surfaces,
vertex normals on surfaces and on the light, many lights, and through a thin lens.

The reference is computed on the CPU and shares nothing with the device (tests/path_ref.py says where each primitive comes from);
tests/test_path_ref_cpu.py holds it to the CPU oracle and shows that these very inputs (tests/path_cases.py) reach every branch
under test with at least 8 paths, and that a branch taken wrongly changes at least 8 of them.  Every comparison here is equality
of bytes: 1024 paths per case, no tolerance, no exempted path."""
from __future__ import annotations

import numpy as np
import pytest

from tests import light_cases as lc, path_cases as pc
from tests.test_gpu_parity import assert_built_where_asked

pytestmark = pytest.mark.gpu

ENGINES = ("megakernel", "wavefront")
# The walker's cap and the survival bound it rests on: path_cases.CAP = 256 vertices.  Russian roulette keeps a path with
# probability min(max3(T) eta^2, 0.99) from depth 3 on -- 0.99 at most, reached only along specular chains and inside the glass;
# the fog's albedo leaves 0.9, a wall 0.725.  The inputs are fixed, so the longest path is a fact: tests/test_path_ref_cpu.py
# asserts that no path of any case, integrator or stream takes more than path_cases.LONGEST vertices, under half the cap, and
# the walker asserts that none is alive at the cap.  Nothing is dropped: a path the device carried further than the reference
# would differ in its bytes.


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1).sum())


@pytest.mark.parametrize("integrator", pc.PATHS)
@pytest.mark.parametrize("case", list(pc.CASES))
def test_paths_equal_the_reference_bit_for_bit(renderer_factory, case, integrator):
    sc = pc.scene_of(case, integrator)
    builder = pc.CASES[case][1]
    r = renderer_factory(sc, builder=builder)
    assert_built_where_asked(r, builder)
    assert (r.medium is not None) == (sc.medium is not None) and (r.environment_size > 0) == (sc.environment is not None)
    if case in pc.OUTSIDE_LDS:
        assert not lc.fits(lc.table_counts(sc))      # wf_shade<..., LDSTAB = false, ...>: the tables are read from memory
    idx, seq, f, rays = pc.inputs(case)
    lens = sc.camera.aperture_radius > 0
    if lens:
        assert r.lens == (float(np.float32(sc.camera.aperture_radius)), float(np.float32(sc.camera.focus_distance)))
        assert r.sample_rays_lens(np.stack([(idx % pc.W).astype(np.float32) + f[:, 0], (idx // pc.W).astype(np.float32) + f[:, 1]], 1), f[:, 2:4]).tobytes() == rays.tobytes()
    else:
        # 1. Li of the stated rays, its stream seeded like the render's and drawn from the start
        want_li, _, _, _ = pc.reference(case, integrator, True)
        got_li = r.li(rays, idx, seq)
        print(case, integrator, "li:", differing(got_li, want_li), "of", pc.N_PATHS, "paths differ")
        assert got_li.tobytes() == want_li.tobytes(), (case, integrator, differing(got_li, want_li))
    # 2. both engines' frames of one sample per pixel under the box filter: a pixel is Li of its path
    want, nc, ns, _ = pc.reference(case, integrator)
    assert (want > 0).any() and nc > pc.N_PATHS and (ns > 0) == (integrator != "path_mats")
    frames = {}
    for engine in ENGINES:
        r.set_option("engine", engine)
        frame, st = r.render_host(spp_count=1, spp_begin=pc.S)
        assert st["engine"] == ENGINES.index(engine) and st["n_camera_samples"] == pc.N_PATHS
        assert frame.shape == (pc.H, pc.W, 4) and (frame[..., 3] == 1).all()
        got = frame[..., :3].reshape(-1, 3)
        print(case, integrator, engine, ":", differing(got, want), "of", pc.N_PATHS, "paths differ; rays", st["n_closest_rays"], st["n_shadow_rays"], "want", nc, ns)
        assert got.tobytes() == want.tobytes(), (case, integrator, engine, differing(got, want))
        assert (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns), (case, integrator, engine)
        assert st["n_invalid"] == 0
        if engine == "wavefront":
            assert st["wf_record"] == "full"      # a fog or a sky: the one general variant, on the full record
        frames[engine] = frame
    # 3. a quarter of the samples in flight: regeneration, many passes, wf_finish
    r.set_option("wavefront_paths", pc.N_PATHS // 4)
    small, st = r.render_host(spp_count=1, spp_begin=pc.S)
    assert st["engine"] == 1 and st["n_invalid"] == 0 and (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns)
    assert small.tobytes() == frames["wavefront"].tobytes(), (case, integrator, differing(small[..., :3].reshape(-1, 3), want))
