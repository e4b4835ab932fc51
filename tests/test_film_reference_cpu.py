"""The binary64 film of the oracle (oracle.h: oracle_render_f64) and the summation bound the GPU film tests hold the
device's frames to (tests/test_gpu_parity.py: assert_within_summation_bound) -- checked here on the oracle's own float32
film, whose summation order is the reference's at threads = 1 and depends on the scheduling of the blocks at threads = 16.
No GPU."""
import numpy as np
import pytest

from nori_amd.scene import RFilter
from tests import film_cases
from tests.backends import Oracle
from tests.test_gpu_parity import assert_within_summation_bound


@pytest.mark.parametrize("name", list(film_cases.ROWS))
def test_float_film_of_the_oracle_is_within_the_summation_bound(name):
    ref = film_cases.row_reference(name)
    w, h, rf, spp = film_cases.ROWS[name]
    total, abs_total, terms = ref.film
    assert ref.frame.shape == total.shape == (h + 2 * ref.border, w + 2 * ref.border, 4)
    assert ref.stats["n_invalid"] == 0 and ref.stats["n_camera_samples"] == w * h * spp
    assert_within_summation_bound(ref.frame, total, abs_total, terms, f"{name}, 1 thread")
    o = Oracle(ref.scene, use_bvh=True)
    F16, st16 = o.render_host(threads=16)
    assert st16["n_closest_rays"] == ref.stats["n_closest_rays"] and st16["n_shadow_rays"] == ref.stats["n_shadow_rays"]
    assert_within_summation_bound(F16, total, abs_total, terms, f"{name}, 16 threads")
    # the binary64 film itself: the same terms whatever the number of threads (their sum to ~2^-53, not to the bit)
    if name[0] in "agi":
        t16, a16, n16, _ = o.render_f64(threads=16)
        assert np.array_equal(n16, terms)
        np.testing.assert_allclose(t16, total, rtol=0, atol=1e-12 * float(abs_total.max()))
        np.testing.assert_allclose(a16, abs_total, rtol=1e-12, atol=0)
    # a sample reaches at most (2 border + 1)^2 pixels; every pixel of the image proper is reached by its own samples
    assert int(terms.max()) <= spp * (2 * ref.border + 1) ** 2
    b = ref.border
    assert int(terms[b:b + h, b:b + w].min()) >= spp
    assert (abs_total >= np.abs(total)).all()
    # W: the terms are the weights themselves
    if rf.type == "box":
        assert np.array_equal(total[..., 3], np.full((h, w), float(spp))) and np.array_equal(ref.frame[..., 3], np.full((h, w), np.float32(spp)))
    if rf.type == "mitchell":
        assert (abs_total[..., 3] > total[..., 3]).any()      # negative lobes
    else:
        assert np.array_equal(abs_total[..., 3], total[..., 3])


def test_the_rows_leave_pixels_without_weight():
    """The exact-zero clause of the bound is exercised: pixels where a channel's terms all vanish (black under every sample
    that reaches them -- the light's surround, the frame's outer ring beside it) exist in every row of 45 x 37 and 33 x 17."""
    n = {name: int((film_cases.row_reference(name).abs_total == 0).any(axis=-1).sum()) for name in film_cases.ROWS}
    print(n)
    assert all(v > 0 for name, v in n.items() if film_cases.ROWS[name][0] >= 33), n


def test_binary64_film_honours_the_render_parameters():
    """tile_mod / tile_rem, spp_begin and the seed mode select the same samples as in oracle_render: the parts add up to the
    whole, term for term, and each part's float frame is within the bound of its own binary64 film."""
    from nori_amd import _capi as capi
    sc = film_cases.cornell(45, 37, 6, RFilter("gaussian"))
    o = Oracle(sc, use_bvh=True)
    whole = o.render_f64(threads=1)
    parts = [o.render_f64(tile_mod=3, tile_rem=k, threads=1) for k in range(3)]
    assert np.array_equal(sum(p[2] for p in parts), whole[2])
    np.testing.assert_allclose(sum(p[0] for p in parts), whole[0], rtol=0, atol=1e-12 * float(whole[1].max()))
    for k, p in enumerate(parts):
        F, _ = o.render_host(tile_mod=3, tile_rem=k, threads=1)
        assert_within_summation_bound(F, p[0], p[1], p[2], f"tile_rem {k} of 3")
    halves = [o.render_f64(spp_count=2, spp_begin=0, threads=1), o.render_f64(spp_count=4, spp_begin=2, threads=1)]
    assert np.array_equal(halves[0][2] + halves[1][2], whole[2])
    np.testing.assert_allclose(halves[0][0] + halves[1][0], whole[0], rtol=0, atol=1e-12 * float(whole[1].max()))
    F, st = o.render_host(seed_mode=capi.SEED_NORI_BLOCK, threads=1)
    t, a, n, st64 = o.render_f64(seed_mode=capi.SEED_NORI_BLOCK, threads=1)
    assert st64["n_closest_rays"] == st["n_closest_rays"] and not np.array_equal(t, whole[0])
    assert_within_summation_bound(F, t, a, n, "reference sampler")


def test_invalid_samples_are_left_out_of_both_films():
    """A light with a negative channel makes samples the isValid() guard rejects: they are counted, and add no term."""
    sc = film_cases.cornell(45, 37, 8, RFilter("gaussian"), "path_mats", radiance=(20.0, -1.0, 20.0))
    o = Oracle(sc, use_bvh=True)
    F, st = o.render_host(threads=1)
    t, a, n, st64 = o.render_f64(threads=1)
    assert 0 < st["n_invalid"] < st["n_camera_samples"] and st64["n_invalid"] == st["n_invalid"]
    assert_within_summation_bound(F, t, a, n, "negative light")
    assert (F >= 0).all()
    clean = Oracle(film_cases.cornell(45, 37, 8, RFilter("gaussian"), "path_mats"), use_bvh=True).render_f64(threads=1)[2]
    assert int(clean.sum()) > int(n.sum()) and (clean >= n).all()


def test_bound_helper_rejects_what_it_should():
    """One ulp-scale nudge passes, an error of the size of one dropped or doubled term does not; a value where nothing
    has weight must be 0."""
    ref = film_cases.row_reference("a-one-past-a-chunk")
    total, abs_total, terms = ref.film
    assert_within_summation_bound(np.where(ref.frame != 0, np.nextafter(ref.frame, np.float32(np.inf)), ref.frame), total, abs_total, terms, "one ulp up")
    y, x = np.unravel_index(np.argmax(terms), terms.shape)
    F = ref.frame.copy(); F[y, x, 3] *= np.float32(1 + 1.0 / 256)
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within_summation_bound(F, total, abs_total, terms, "a pixel 0.4 % off")
    F = ref.frame.copy(); F[tuple(np.argwhere(abs_total == 0)[0])] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="differ from 0"):
        assert_within_summation_bound(F, total, abs_total, terms, "weight from nowhere")
