"""The operands and references of tests/arith_cases.py, checked before they judge a kernel (tests/test_gpu_arith.py): numpy's
float32 operations are the IEEE ones, the classes of quotients are what they claim to be and survive the domain filter, the
domains are the header's, and the two CPU implementations of the specified transcendentals agree on the new argument sets."""
import os

import numpy as np

from tests import arith_cases as ac
from tests.arith_cases import F, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _once(f, *xs):
    """the binary64 operation rounded once to binary32: for + - * / sqrt, 53 >= 2 * 24 + 2 bits make the double rounding innocuous"""
    with np.errstate(all="ignore"):
        return f(*[x.astype(np.float64) for x in xs]).astype(F)


def test_numpy_float32_reciprocal_quotient_and_root_are_ieee():
    n = 0
    for _, x in ac.rcp_chunks():
        assert np.array_equal(bits(ac.rcp_ref(x)), bits(_once(lambda v: 1.0 / v, x)))
        n += x.size
    assert n == 6 * (1 << 23) + 2 * 4096 * (252 - 3)
    d = ac.div_cases()
    for a, b in ac.chunks(d.a, d.b):
        assert np.array_equal(bits(ac.div_ref(a, b)), bits(_once(lambda u, v: u / v, a, b)))
    for _, x in ac.sqrt_cases():
        assert np.array_equal(bits(ac.sqrt_ref(x)), bits(_once(np.sqrt, x)))
    assert bits(ac.sqrt_ref(F(-0.0)))[0] == 0x80000000


def test_every_case_lies_inside_its_domain_and_the_filter_hides_no_class():
    for _, x in ac.rcp_chunks():
        assert x.size <= ac.CHUNK and ac.in_rcp_domain(x).all()
    for _, x in ac.sqrt_cases():
        assert ac.in_sqrt_domain(x).all()
    assert sum(x.size for _, x in ac.sqrt_cases()) >= (1 << 24) + 232 * 4096 + 4096 + 4
    d = ac.div_cases()
    assert ac.in_div_domain(d.a, d.b, ac.div_ref(d.a, d.b)).all()
    assert (1 << 24) <= d.a.size <= (1 << 24) + (1 << 20)      # "about 2^24 pairs"
    for c, name in enumerate(ac.DIV_CLASSES):
        assert d.kept[c] == int((d.cls == c).sum()) and d.generated[c] > 0
        print(f"[arith] div class {name}: generated {d.generated[c]}, kept {d.kept[c]} ({d.kept[c] / d.generated[c]:.1%})")
        assert d.kept[c] >= ac.DIV_KEEP[name] * d.generated[c], (name, int(d.kept[c]), int(d.generated[c]))
    # the exponents of class (a) reach the ends of the stated domain, far beyond +-60
    a, b = d.a[d.cls == 0], d.b[d.cls == 0]
    ea, eb = ((bits(a) >> 23) & 0xFF).astype(int) - 127, ((bits(b) >> 23) & 0xFF).astype(int) - 127
    assert eb.min() == -126 and eb.max() == 125 and ea.min() == -100 and ea.max() == 127
    assert (ea - eb).min() == -125 and (ea - eb).max() == 127
    # the zero numerators: all four sign pairs, equally often
    z = d.cls == 3
    pairs = (bits(d.a[z]) >> 31) * 2 + (bits(d.b[z]) >> 31)
    assert (d.a[z] == 0).all() and np.array_equal(np.bincount(pairs, minlength=4), [1 << 14] * 4)


def test_hard_quotients_lie_next_to_a_midpoint():
    """Class (c): |A / B - midpoint| = |delta| / (2 B) ulp, at most 3 / 2^24 ulp = 1.8e-7 ulp; measured in binary64 (whose own error,
    2^-53 relative, is 2^-29 ulp of the float32 quotient): at most 2^-22 ulp for every kept pair."""
    d = ac.div_cases()
    c = d.cls == 2
    A = ((bits(d.a[c]) & 0x7FFFFF) | 0x800000).astype(np.float64)
    B = ((bits(d.b[c]) & 0x7FFFFF) | 0x800000).astype(np.float64)
    assert A.size >= 1 << 20 and (A < B).all()
    t = (A / B) * 2.0 ** 24                       # in [2^23, 2^24): one float32 ulp of the quotient is 1
    dist = np.abs((t - np.floor(t)) - 0.5)
    print(f"[arith] class (c): {A.size} pairs, distance to a midpoint at most {dist.max():.3g} ulp")
    assert dist.max() <= 2.0 ** -22
    # and the construction itself, on fresh draws: exact in integers
    A, B, delta = ac.hard_quotients(np.random.default_rng(7), 1 << 16)
    assert A.size >= 0.25 * (1 << 16)
    M2 = (A * (1 << 25) + delta)                  # = B M
    assert (M2 % B == 0).all() and ((M2 // B) % 2 == 1).all() and ((M2 // B) >= (1 << 24)).all() and ((M2 // B) < (1 << 25)).all()


def test_domain_predicates_agree_with_the_header_at_every_edge():
    up = lambda x: np.nextafter(F(x), F(np.inf))
    dn = lambda x: np.nextafter(F(x), F(-np.inf))
    header = open(os.path.join(ROOT, "nori_amd", "csrc", "device", "rt_types.h")).read()
    # the numbers the header's conditions are written with are the powers of two of its prose
    for text, value in (("1.17549435e-38f", 2.0 ** -126), ("8.5070592e37f", 2.0 ** 126), ("7.8886091e-31f", 2.0 ** -100), ("4.9303807e-32f", 2.0 ** -104),
                        ("3.4028235e38f", float(ac.FLT_MAX))):
        assert text in header and F(float(text[:-1])) == F(value), text
    for s in (F(1), F(-1)):
        assert ac.in_rcp_domain(s * F(2.0 ** -126)) and not ac.in_rcp_domain(s * dn(2.0 ** -126))
        assert ac.in_rcp_domain(s * dn(2.0 ** 126)) and not ac.in_rcp_domain(s * F(2.0 ** 126))
    assert not ac.in_rcp_domain(F(0)) and not ac.in_rcp_domain(F(np.inf)) and not ac.in_rcp_domain(F(np.nan))

    def div_in(a, b):
        a, b = np.array([a], F), np.array([b], F)
        return bool(ac.in_div_domain(a, b, ac.div_ref(a, b))[0])
    assert div_in(1, 2.0 ** -126) and not div_in(2.0 ** -100, dn(2.0 ** -126))
    assert div_in(2.0 ** 100, dn(2.0 ** 126)) and not div_in(2.0 ** 100, 2.0 ** 126)
    assert div_in(2.0 ** -100, 1) and not div_in(dn(2.0 ** -100), 1) and div_in(0.0, 1) and div_in(-0.0, -1) and not div_in(0.0, 0.0)
    assert div_in(2.0 ** -100, 2.0 ** 26) and not div_in(2.0 ** -100, up(2.0 ** 26))          # the quotient 2^-126 and the denormal below it
    assert div_in(dn(ac.FLT_MAX), 1) and not div_in(ac.FLT_MAX, 1) and not div_in(2.0 ** 127, 0.5)      # below FLT_MAX; FLT_MAX; overflow
    assert not div_in(np.inf, 1) and not div_in(np.nan, 1)
    a, b = ac.div_outside_top()
    q = ac.div_ref(a, b)
    assert (q == ac.FLT_MAX).all() and not ac.in_div_domain(a, b, q).any()
    assert ac.in_sqrt_domain(F(2.0 ** -104)) and not ac.in_sqrt_domain(dn(2.0 ** -104))
    assert ac.in_sqrt_domain(F(0.0)) and ac.in_sqrt_domain(F(-0.0)) and ac.in_sqrt_domain(F(np.inf)) and ac.in_sqrt_domain(ac.FLT_MAX)
    assert not ac.in_sqrt_domain(F(-1)) and not ac.in_sqrt_domain(F(np.nan)) and not ac.in_sqrt_domain(F(1e-45))


def test_the_stated_contract_of_a_zero_numerator():
    """div_contract is IEEE's quotient except for the one case the header names: -0 / b, b > 0, is +0."""
    d = ac.div_cases()
    want, ieee = ac.div_contract(d.a, d.b), ac.div_ref(d.a, d.b)
    differ = bits(want) != bits(ieee)
    assert int(differ.sum()) == 1 << 14 and (d.cls[differ] == 3).all()
    assert (bits(d.a[differ]) == 0x80000000).all() and (d.b[differ] > 0).all() and (bits(want[differ]) == 0).all() and (bits(ieee[differ]) == 0x80000000).all()
    z = np.array([0.0, 0.0, -0.0, -0.0], F); b = np.array([3.0, -3.0, 3.0, -3.0], F)
    assert np.array_equal(bits(ac.div_contract(z, b)), np.array([0, 0x80000000, 0, 0], np.uint32))


def test_slab_reference_and_its_operands():
    d = ac.slab_cases()
    want = ac.slab_ref(d)
    exact = np.abs(d) >= F(2.0 ** -60)
    assert np.array_equal(bits(want[exact]), bits(ac.rcp_ref(d[exact])))
    assert np.array_equal(bits(want[~exact]), np.where(bits(d[~exact]) >> 31, bits(-ac.TWO60), bits(ac.TWO60)).astype(np.uint32))
    e = ((bits(d) >> 23) & 0xFF).astype(int)
    assert set(e) == set(range(0, 253)) and (bits(d) == 0).any() and (bits(d) == 0x80000000).any()      # zeros, denormals, every exponent below 2^126
    for s in (F(1), F(-1)):
        for v in (F(2.0 ** -60), np.nextafter(F(2.0 ** -60), F(0)), np.nextafter(F(2.0 ** -60), F(1))):
            assert (d == s * v).any()
    assert int(exact.sum()) > 1000 and int((~exact).sum()) > 1000


def test_emulated_and_oracle_transcendentals_agree_on_the_new_argument_sets():
    """rt_math.h (compiled for the CPU) and oracle_libm.h on every argument set the GPU test uses, the quadrant and cancellation
    bands included; and both equal the correctly rounded value where tests/test_device_logic_cpu.py claims it."""
    from tests.backends import Emu, Oracle
    for op in ("sin", "cos", "log", "exp"):
        for label, x, cr in ac.libm_cases(op):
            o = Oracle.libm(op, x)
            assert np.array_equal(bits(o), bits(Emu.libm(op, x))), (op, label)
            if cr:
                assert np.array_equal(bits(o), bits(ac.correctly_rounded(op, x))), (op, label)
            if op in ("sin", "cos"):
                assert (np.abs(x) <= F(2.0 ** 20)).all()
    edges = [x for label, x, _ in ac.libm_cases("exp") if label == "edges"][0]
    assert np.array_equal(bits(Oracle.libm("exp", edges)), bits(ac.EXP_EDGES_EXPECTED))
    sets = {label: x for label, x, _ in ac.libm_cases("sin")}
    assert sets["all of [2^-12, 2^-10]"].size == (1 << 24) + 1 and sets["band around pi"].size == 4097
    assert [x for label, x, _ in ac.libm_cases("log") if label.startswith("all of")][0].size == (1 << 14) + 1


def test_counter_operands_keep_away_from_the_borders():
    """The operands of tools/arith_excursion_probe.py: every one outside a domain stays outside when moved a factor 4 towards it, and
    every quotient inside stays inside when moved a factor 4 towards either end -- so the library's own condition (which judges the
    quotient from the device's estimate) and the predicates here must count the same operands.  Each count is non-zero: a
    condition that never fires cannot pass."""
    c = ac.counter_cases()
    want = ac.counter_expectation(c)
    assert min(want) >= 400 and max(c.rcp.size, c.sqrt.size, c.div_a.size) < 8192
    out = ~ac.in_rcp_domain(c.rcp)
    assert (~ac.in_rcp_domain(c.rcp[out] * F(4))).all() and (~ac.in_rcp_domain(c.rcp[out] * F(0.25))).all()
    out = ~ac.in_sqrt_domain(c.sqrt)
    assert (c.sqrt[out] > 0).all() and (~ac.in_sqrt_domain(c.sqrt[out] * F(4))).all()
    a, b = c.div_a, c.div_b
    ok = ac.in_div_domain(a, b, ac.div_ref(a, b))
    with np.errstate(all="ignore"):
        q64 = np.abs(a.astype(np.float64) / b.astype(np.float64))
    for s in (4.0, 0.25):
        q = q64 * s
        assert (((q >= 2.0 ** -126) & (q < float(ac.FLT_MAX)))[ok & (a != 0)]).all()
        bad_q = ~ok & ac.in_rcp_domain(b) & (np.abs(a) >= F(2.0 ** -100))      # outside because of the quotient alone
        assert bad_q.sum() >= 200 and (~((q >= F(2.0 ** -126)) & (q < ac.FLT_MAX))[bad_q]).all()
    assert ac.in_rcp_domain(c.inside["rcp"]).all() and ac.in_sqrt_domain(c.inside["sqrt"]).all()
    ia, ib = c.inside["div"]
    assert ac.in_div_domain(ia, ib, ac.div_ref(ia, ib)).all() and np.isfinite(ac.div_ref(ia, ib)).all()
