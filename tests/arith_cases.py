"""Operands and references for the device's own arithmetic (nori_amd/csrc/device/rt_types.h: exact_rcp, exact_div, the shared
reciprocal of f3 / float, exact_sqrt; rt_trace.h: slab_rcp; rt_math.h: det_sincosf, det_logf, det_expf), shared by
tests/test_arith_cases_cpu.py -- which checks the generators and the references themselves -- and tests/test_gpu_arith.py,
which then holds the device to them through Renderer.arith.  numpy only; fixed seeds; every comparison is on BIT PATTERNS
(bits()), never `==` on floats: -0 and +0 are different results.

The domains below are written from the prose of the rt_types.h header, not from its NORI_EXCURSION conditions (those are
code under test):
    exact_rcp(x)     2^-126 <= |x| < 2^126
    exact_div(a, b)  b as for exact_rcp;  a = 0, or |a| >= 2^-100 with a / b a normal number below the largest finite float
    exact_sqrt(x)    x = 0, x = +inf, or x >= 2^-104
Outside them the last bit is unspecified and nothing is asserted, except for slab_rcp, which is defined everywhere:
    slab_rcp(d) = copysign(min(|1 / d|, 2^60), d)
(the sequence is exact where |d| >= 2^-60 and clamps every reciprocal beyond 2^60; a zero or denormal d comes back from the
Newton step infinite or NaN, fails the `<=` and is clamped too).

One departure from IEEE inside exact_div's domain is part of its contract (rt_types.h): a ZERO numerator
gives a zero of IEEE's sign except for -0 / b with b > 0, which gives +0 (div_contract).
"""
from __future__ import annotations

import functools

import numpy as np

F, U = np.float32, np.uint32
CHUNK = 1 << 22      # elements per device call: the library stages operands and results in scratch buffers of this many floats
FLT_MAX = F(3.4028234663852886e38)
TWO60 = F(2.0 ** 60)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U)


def floats(u):
    return np.ascontiguousarray(u, dtype=U).view(F)


def pack(sign, e, mant):
    """float32 of a sign bit, an UNBIASED exponent (-126 .. 127; -127 gives the zero / denormal encoding) and a mantissa field"""
    s, e, m = np.broadcast_arrays(np.asarray(sign, np.int64), np.asarray(e, np.int64), np.asarray(mant, np.int64))
    assert ((e >= -127) & (e <= 127)).all() and ((m >= 0) & (m < (1 << 23))).all() and ((s == 0) | (s == 1)).all()
    return floats((s << 31) | ((e + 127) << 23) | m)


# the mantissa fields next to all-zeros and next to all-ones: where a reciprocal's or a quotient's error is largest (the cases
# tools/ubench_divsqrt.hip mixes in)
PATTERNS = np.concatenate([np.arange(16), 0x7FFFFF - np.arange(16)]).astype(np.int64)


def mantissas(rng, n):
    """n mantissa fields: the 32 PATTERNS, the rest random"""
    assert n >= 64
    return np.concatenate([PATTERNS, rng.integers(0, 1 << 23, n - PATTERNS.size)])


def chunks(*arrays):
    """the arrays in slices of at most CHUNK elements"""
    n = arrays[0].size
    for i in range(0, n, CHUNK):
        yield tuple(a[i:i + CHUNK] for a in arrays)


# ------------------------------------------------------------------------------------------------ domains (header prose)
def in_rcp_domain(x):
    ax = np.abs(np.asarray(x, F))
    return (ax >= F(2.0 ** -126)) & (ax < F(2.0 ** 126))


def in_div_domain(a, b, q):
    """q: the REFERENCE quotient a / b in float32 (the filter must not look at what the device returns)"""
    a, b, q = np.asarray(a, F), np.asarray(b, F), np.asarray(q, F)
    aq = np.abs(q)
    return in_rcp_domain(b) & ((a == 0) | ((np.abs(a) >= F(2.0 ** -100)) & np.isfinite(a) & (aq >= F(2.0 ** -126)) & (aq < FLT_MAX)))


def in_sqrt_domain(x):
    x = np.asarray(x, F)
    return (x == 0) | (x >= F(2.0 ** -104))      # +inf included, NaN and negative numbers not


# ------------------------------------------------------------------------------------------------------------ references
def rcp_ref(x):
    with np.errstate(all="ignore"):
        return F(1) / np.asarray(x, F)


def div_ref(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, F) / np.asarray(b, F)


def div_contract(a, b):
    """What exact_div is specified to return inside its domain: a / b, bit for bit, except that -0 / b is +0 for b > 0."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    q = div_ref(a, b).copy()
    q[(bits(a) == U(0x80000000)) & (b > 0)] = F(0.0)
    return q


def sqrt_ref(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, F))


def slab_ref(d):
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        return np.copysign(np.minimum(np.abs(F(1) / d), TWO60), d)


# ------------------------------------------------------------------------------------------------------------ reciprocal
RCP_FULL_EXPONENTS = (0, -126, 125)      # the middle and the two ends of [2^-126, 2^126): all 2^23 mantissas, both signs


def rcp_chunks():
    """(label, x) with at most CHUNK operands each, all inside the domain: every mantissa at RCP_FULL_EXPONENTS, 4096 mantissas
    (PATTERNS + random) at every other exponent of the domain, both signs."""
    all_m = np.arange(1 << 23, dtype=np.int64)
    for e in RCP_FULL_EXPONENTS:
        for s in (0, 1):
            for (m,) in chunks(all_m):
                yield f"2^{e} all mantissas sign {s}", pack(s, e, m)
    rng = np.random.default_rng(101)
    xs = []
    for e in range(-126, 126):
        if e not in RCP_FULL_EXPONENTS:
            m = mantissas(rng, 4096)
            xs += [pack(0, e, m), pack(1, e, m)]
    for (x,) in chunks(np.concatenate(xs)):
        yield "4096 mantissas at every other exponent", x


# ----------------------------------------------------------------------------------------------------------- square root
@functools.lru_cache(maxsize=None)
def sqrt_cases():
    """[(label, x)]: every float of [1, 4) -- inside the domain nothing scales, so the result depends on the mantissa and on the
    exponent's parity only: this is exhaustive over what can differ --, 4096 mantissas at every exponent from 2^-104 to the
    largest finite, the squares of the integers below 4096, and +0, -0, +inf, 2^-104."""
    rng = np.random.default_rng(102)
    rows = [("all of [1, 4)", floats(np.arange(0x3F800000, 0x40800000, dtype=np.int64)))]
    rows.append(("4096 mantissas at every exponent", np.concatenate([pack(0, e, mantissas(rng, 4096)) for e in range(-104, 128)])))
    k = np.arange(4096, dtype=np.int64)
    rows.append(("perfect squares", (k * k).astype(F)))      # < 2^24: exact
    rows.append(("zeros, infinity, 2^-104", np.array([0.0, -0.0, np.inf, 2.0 ** -104], F)))
    for _, x in rows:
        x.setflags(write=False)
    return rows


# -------------------------------------------------------------------------------------------------------------- slab_rcp
@functools.lru_cache(maxsize=None)
def slab_cases():
    """d over every exponent below 2^126, both signs; +-0; denormals; 2^-60 (the largest reciprocal that is not clamped) and its
    two neighbours."""
    rng = np.random.default_rng(103)
    xs = [pack(s, e, mantissas(rng, 1024)) for e in range(-126, 126) for s in (0, 1)]
    den = np.concatenate([mantissas(rng, 4096), [1, 2, 0x400000]])
    den = den[den != 0]
    xs += [pack(0, -127, den), pack(1, -127, den)]
    edge = bits(np.array([2.0 ** -60], F)).astype(np.int64)[0]
    e6 = floats(np.array([edge - 1, edge, edge + 1], np.int64))
    xs += [np.array([0.0, -0.0], F), e6, -e6]
    x = np.concatenate(xs)
    x.setflags(write=False)
    return x


# -------------------------------------------------------------------------------------------------------------- quotient
DIV_CLASSES = ("a-whole-domain", "b-mantissa-patterns", "c-next-to-a-midpoint", "d-zero-numerator", "e-integer-quotients", "f-domain-edges")
DIV_KEEP = {name: 0.90 for name in DIV_CLASSES}      # the share of what a class GENERATES that the domain filter must leave
DIV_KEEP["c-next-to-a-midpoint"] = 0.25              # of its DRAWS: the construction itself rejects two thirds


def _exponents(rng, n):
    """(ea, eb): eb over the whole domain of the divisor, then ea - eb over everything that leaves |a| >= 2^-100, a finite and the
    quotient normal whatever the mantissas are (its exponent is ea - eb or ea - eb - 1).  Drawing the quotient's exponent, not
    both operands', is what lets the classes cover the whole domain and still pass the filter."""
    eb = rng.integers(-126, 126, n)
    lo, hi = np.maximum(-125, -100 - eb), np.minimum(127, 127 - eb)
    return rng.integers(lo, hi + 1) + eb, eb


def hard_quotients(rng, n):
    """(A, B, delta) of the draws that survive, int64: quotients A / B of 24-bit integers as close to a rounding boundary as a
    quotient of floats can be.  For an odd B and delta in {+-1, +-3}: inv = B^-1 mod 2^25 (Newton steps x <- x (2 - B x) in
    uint64, each doubling the valid bits of x = B, which is right to 3), M = delta inv mod 2^25 -- odd, so M / 2^25 with
    M >= 2^24 is the midpoint of two neighbouring floats of [1/2, 1) --, A = (B M - delta) / 2^25, an integer.  Then
    A / B = (M - delta / B) / 2^25: |delta| / (2 B) ulp away from that midpoint.  A draw is kept if M >= 2^24 and
    2^23 <= A < 2^24."""
    B = (rng.integers(1 << 22, 1 << 23, n) * 2 + 1).astype(np.uint64)
    delta = rng.choice(np.array([1, -1, 3, -3], np.int64), n)
    x = B.copy()
    for _ in range(5):
        x = x * (np.uint64(2) - B * x)      # mod 2^64
    mask = np.uint64((1 << 25) - 1)
    assert ((B * x) & mask == 1).all()
    M = ((delta.astype(np.uint64) * x) & mask).astype(np.int64)      # two's complement: -1 is 2^64 - 1
    Bi = B.astype(np.int64)
    num = Bi * M - delta
    assert (num % (1 << 25) == 0).all()
    A = num >> 25
    keep = (M >= (1 << 24)) & (A >= (1 << 23)) & (A < (1 << 24))
    return A[keep], Bi[keep], delta[keep]


class DivCases:
    """a, b (float32), cls (index into DIV_CLASSES) of the pairs inside exact_div's domain; generated[c] / kept[c] per class."""


@functools.lru_cache(maxsize=None)
def div_cases() -> DivCases:
    rng = np.random.default_rng(104)
    parts = []          # (class index, a, b, how many draws these stand for)

    def sign(n):
        return rng.integers(0, 2, n)

    # (a) random mantissas, exponents over the whole stated domain
    n = 12 << 20
    ea, eb = _exponents(rng, n)
    parts.append((0, pack(sign(n), ea, rng.integers(0, 1 << 23, n)), pack(sign(n), eb, rng.integers(0, 1 << 23, n)), n))
    # (b) mantissas next to all-ones / all-zeros in the divisor, the numerator, or both
    n = 2 << 20
    ea, eb = _exponents(rng, n)
    ma, mb, sel = rng.integers(0, 1 << 23, n), rng.integers(0, 1 << 23, n), rng.integers(0, 6, n)
    pa, pb = rng.integers(0, 16, n), rng.integers(0, 16, n)
    mb = np.where((sel == 0) | (sel == 4), 0x7FFFFF - pb, np.where((sel == 1) | (sel == 5), pb, mb))
    ma = np.where((sel == 2) | (sel == 5), 0x7FFFFF - pa, np.where((sel == 3) | (sel == 4), pa, ma))
    parts.append((1, pack(sign(n), ea, ma), pack(sign(n), eb, mb), n))
    # (c) quotients next to a rounding boundary
    n = 4 << 20
    A, B, _ = hard_quotients(rng, n)
    ea, eb = _exponents(rng, A.size)
    parts.append((2, pack(sign(A.size), ea, A - (1 << 23)), pack(sign(A.size), eb, B - (1 << 23)), n))
    # (d) +-0 over +-b
    n = 1 << 14
    b = pack(0, rng.integers(-126, 126, n), mantissas(rng, n))
    z = np.zeros(n, F)
    for za in (z, -z):
        for bb in (b, -b):
            parts.append((3, za, bb, n))
    # (e) a = +-k b for k = 1 (a == b) .. 17; the divisor's low five mantissa bits are clear, so k b is exact
    n = 1 << 14
    for k in range(1, 18):
        b = pack(sign(n), rng.integers(-100, 121, n), mantissas(rng, n) & ~0x1F)
        a = (F(k) * b) * np.where(sign(n) == 1, F(-1), F(1))
        assert np.array_equal(np.abs(a).astype(np.float64), k * np.abs(b).astype(np.float64))
        parts.append((4, a, b, n))
    # (f) the edges of the domain
    n = 1 << 16
    parts.append((5, pack(sign(n), -100, 0), pack(sign(n), rng.integers(-126, 26, n), mantissas(rng, n)), n))          # |a| = 2^-100
    parts.append((5, pack(sign(n), rng.integers(-100, 2, n), mantissas(rng, n)), pack(sign(n), -126, 0), n))           # b = 2^-126
    parts.append((5, pack(sign(n), rng.integers(1, 128, n), mantissas(rng, n)), pack(sign(n), 125, 0x7FFFFF), n))      # b the largest below 2^126
    m1, m2 = mantissas(rng, n), mantissas(rng, n)[::-1]
    lo_m, hi_m = np.minimum(m1, m2), np.maximum(m1, m2)
    lo_m = np.where(lo_m == hi_m, 0, lo_m); hi_m = np.where(hi_m == 0, 1, hi_m)      # strictly smaller
    eb = rng.integers(26, 126, n)
    parts.append((5, pack(sign(n), eb - 125, lo_m), pack(sign(n), eb, hi_m), n))      # the lowest normal binade: 2^-125 times a ratio below 1
    parts.append((5, pack(sign(n), eb - 126, hi_m), pack(sign(n), eb, lo_m), n))      #                           2^-126 times a ratio of at least 1
    eb = rng.integers(-126, 1, n)
    parts.append((5, pack(sign(n), eb + 127, hi_m), pack(sign(n), eb, lo_m), n))      # the highest normal binade
    eb = rng.integers(-126, 0, n)
    parts.append((5, pack(sign(n), eb + 128, lo_m), pack(sign(n), eb, hi_m), n))
    # ... and its top: quotients 2 .. 17 ulp below 2^128, i.e. 1 .. 16 ulp below the largest finite float.  With eps = 2^-24,
    # b = (1 - j eps) 2^(eb + 1) and a = (1 - (k + 1) eps) 2^(ea + 1): a / b = 2^128 (1 - (k + 1 - j) eps - ...)
    j, t, eb = np.meshgrid(np.arange(1, 17), np.arange(1, 17), np.arange(-126, 0), indexing="ij")
    j, t, eb = j.ravel(), t.ravel(), eb.ravel()
    parts.append((5, pack(sign(j.size), eb + 128, 0x7FFFFF - (j + t)), pack(sign(j.size), eb, 0x7FFFFF - (j - 1)), j.size))

    out = DivCases()
    out.generated = np.zeros(len(DIV_CLASSES), np.int64)
    out.kept = np.zeros(len(DIV_CLASSES), np.int64)
    aa, bb, cc = [], [], []
    for c, a, b, drawn in parts:
        ok = in_div_domain(a, b, div_ref(a, b))
        out.generated[c] += drawn
        out.kept[c] += int(ok.sum())
        aa.append(a[ok]); bb.append(b[ok]); cc.append(np.full(int(ok.sum()), c, np.uint8))
    out.a, out.b, out.cls = np.concatenate(aa), np.concatenate(bb), np.concatenate(cc)
    for arr in (out.a, out.b, out.cls, out.generated, out.kept):
        arr.setflags(write=False)
    return out


def div_outside_top():
    """(a, b) just OUTSIDE the domain at its top: quotients whose correctly rounded value is the largest finite float (the
    k + 1 - j = 1 line of the construction in div_cases).  The estimate a * rcp(b) of such a quotient can round to infinity and
    the sequence then returns NaN where IEEE returns FLT_MAX -- why the domain ends below FLT_MAX.  Nothing is asserted about
    them on the device; tests/test_arith_cases_cpu.py checks that the filter puts them outside."""
    j, eb = np.meshgrid(np.arange(1, 17), np.arange(-126, 0), indexing="ij")
    j, eb = j.ravel(), eb.ravel()
    return pack(0, eb + 128, 0x7FFFFF - j), pack(0, eb, 0x7FFFFF - (j - 1))


# ------------------------------------------------------------------------------------------------------ sin cos log exp
LIBM_N = 1 << 20      # per distribution; tests/test_device_logic_cpu.py::test_specified_transcendentals draws 4 M of each on the CPU


def _between(lo, hi):
    """every float32 of [lo, hi], 0 <= lo <= hi"""
    lo, hi = int(bits(np.array([lo], F))[0]), int(bits(np.array([hi], F))[0])
    assert 0 <= lo <= hi < 0x7F800000
    return floats(np.arange(lo, hi + 1, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def libm_cases(op):
    """[(label, x, correctly_rounded)] for op in sin, cos, log, exp.  Every set is held to Oracle.libm bit for bit; where
    `correctly_rounded`, also to f(float64(x)) rounded once to float32 -- on the ranges for which
    test_specified_transcendentals asserts that of the CPU compilation.

    sin / cos: |x| <= 2^20 (beyond that the quadrant's conversion to an integer is not defined the same way on both sides, and the
    renderer never gets there).  The quadrant switches: every float of the 2^-10-wide bands around pi/4, pi/2, pi, 3pi/2, 2pi;
    at zero every float of [2^-12, 2^-10] -- 2^24 of them: the two binades in which sin x stops rounding to x and cos x to 1 --
    and 4096 mantissas at every exponent below, denormals and both zeros (ALL floats of [0, 2^-10] are 2^30, minutes of
    reference on one core).
    log: every float of [1 - 2^-10, 1], the cancellation end of log(1 - u)."""
    rng = np.random.default_rng({"sin": 105, "cos": 106, "log": 107, "exp": 108}[op])
    n = LIBM_N
    rows = []
    if op in ("sin", "cos"):
        rows.append(("uniform [0, 2pi)", rng.uniform(0, 2 * np.pi, n).astype(F), True))
        if op == "sin":
            rows.append(("uniform [-50, 50)", rng.uniform(-50, 50, 100000).astype(F), True))
        big = (rng.uniform(-1, 1, 1 << 16) * np.exp2(rng.uniform(0, 20, 1 << 16))).astype(F)
        rows.append(("any sign, up to 2^20", big[np.abs(big) <= F(2.0 ** 20)], False))
        for name, c in (("pi/4", np.pi / 4), ("pi/2", np.pi / 2), ("pi", np.pi), ("3pi/2", 1.5 * np.pi), ("2pi", 2 * np.pi)):
            rows.append((f"band around {name}", _between(c - 2.0 ** -11, c + 2.0 ** -11), False))
        rows.append(("all of [2^-12, 2^-10]", _between(2.0 ** -12, 2.0 ** -10), False))
        small = [pack(0, e, mantissas(rng, 4096)) for e in range(-126, -12)] + [pack(0, -127, mantissas(rng, 4096))]
        rows.append(("below 2^-12, denormals, zeros", np.concatenate(small + [np.array([0.0, -0.0], F)]), False))
    elif op == "log":
        rows.append(("1 - uniform [0, 1)", (1.0 - rng.uniform(0, 1, n)).astype(F), True))
        rows.append(("uniform [1e-30, 1e30)", rng.uniform(1e-30, 1e30, n).astype(F), True))
        rows.append(("all of [1 - 2^-10, 1]", _between(1.0 - 2.0 ** -10, 1.0), False))
        rows.append(("edges", np.array([0.0, 1.0, np.inf, 1e-45, 3.4e38], F), True))
    elif op == "exp":
        rows.append(("-exponential(8)", (-rng.exponential(8.0, n)).astype(F), True))
        rows.append(("uniform [-104, 88)", rng.uniform(-104, 88, n).astype(F), True))
        rows.append(("edges", np.array([-200, -104.5, 0, 89, 1e9], F), False))
    else:
        raise KeyError(op)
    out = []
    for label, x, cr in rows:
        x = x[np.isfinite(x) | (label == "edges")]
        if op == "log" and label != "edges":
            x = x[x > 0]
        x = np.ascontiguousarray(x)
        x.setflags(write=False)
        out.append((label, x, cr))
    return out


EXP_EDGES_EXPECTED = np.array([0, 0, 1, np.inf, np.inf], F)      # of the "edges" row of exp, as test_specified_transcendentals states them


def correctly_rounded(op, x):
    f = {"sin": np.sin, "cos": np.cos, "log": np.log, "exp": np.exp}[op]
    with np.errstate(all="ignore"):
        return f(np.asarray(x, F).astype(np.float64)).astype(F)


# ------------------------------------------------------------------------------------------------- the counters' operands
class CounterCases:
    """Operands for tools/arith_excursion_probe.py: a few thousand per sequence of which a KNOWN number lie outside its domain, every
    one of those at least a factor 4 away from the border (the library's condition for the quotient judges it from the device's
    own estimate a * rcp(b), which may differ from a / b in the last bits).  `inside` holds in-domain operands only."""


@functools.lru_cache(maxsize=None)
def counter_cases() -> CounterCases:
    rng = np.random.default_rng(109)
    n = 4096
    c = CounterCases()

    def sgn(k):
        return rng.integers(0, 2, k)

    good = pack(sgn(n), rng.integers(-120, 120, n), mantissas(rng, n))
    # reciprocal: denormals below 2^-128, zeros, and the only magnitude from 2^128 on, infinity
    bad = np.concatenate([pack(sgn(300), -127, rng.integers(1, 1 << 21, 300)), np.where(sgn(200) == 1, F(np.inf), F(-np.inf)), np.array([0.0, -0.0], F)])
    c.rcp = rng.permutation(np.concatenate([good, bad])).astype(F)
    # square root: positive numbers below 2^-106 (denormals among them) are outside; zeros and infinity are inside
    bad = np.concatenate([pack(0, rng.integers(-126, -106, 400), mantissas(rng, 400)), pack(0, -127, rng.integers(1, 1 << 23, 100))])
    good = np.concatenate([pack(0, rng.integers(-102, 128, n), mantissas(rng, n)), np.array([0.0, -0.0, np.inf, 2.0 ** -104], F)])
    c.sqrt = rng.permutation(np.concatenate([good, bad])).astype(F)
    # quotient: in-domain pairs; divisors outside (zero, denormal < 2^-128, infinite); numerators 0 < |a| <= 2^-102; quotients
    # of at most 2^-128 and of at least 2^130 (the estimate overflows)
    ea, eb = _exponents(rng, n)
    keep = (ea - eb > -120) & (ea - eb < 120)
    ga, gb = pack(sgn(n), ea, mantissas(rng, n))[keep], pack(sgn(n), eb, mantissas(rng, n))[keep]
    k = 128
    one = pack(sgn(k), rng.integers(-20, 20, k), mantissas(rng, k))
    ba = [one, one, one, pack(sgn(k), rng.integers(-126, -102, k), mantissas(rng, k)), pack(sgn(k), rng.integers(-90, -70, k), mantissas(rng, k)),
          pack(sgn(k), rng.integers(100, 128, k), mantissas(rng, k)), np.zeros(k, F)]
    bb = [np.zeros(k, F), pack(sgn(k), -127, rng.integers(1, 1 << 21, k)), np.where(sgn(k) == 1, F(np.inf), F(-np.inf)), pack(sgn(k), rng.integers(-20, 20, k), mantissas(rng, k)),
          pack(sgn(k), rng.integers(60, 126, k), mantissas(rng, k)), pack(sgn(k), rng.integers(-126, -32, k), mantissas(rng, k)), np.zeros(k, F)]
    perm = rng.permutation(ga.size + 7 * k)
    c.div_a, c.div_b = np.concatenate([ga] + ba)[perm].astype(F), np.concatenate([gb] + bb)[perm].astype(F)
    c.inside = {"rcp": c.rcp[in_rcp_domain(c.rcp)], "sqrt": c.sqrt[in_sqrt_domain(c.sqrt)]}
    ok = in_div_domain(c.div_a, c.div_b, div_ref(c.div_a, c.div_b))
    c.inside["div"] = (c.div_a[ok], c.div_b[ok])
    return c


def counter_expectation(c: CounterCases):
    """(operands outside the domain of rcp, div, sqrt) by the predicates above"""
    return (int((~in_rcp_domain(c.rcp)).sum()), int((~in_div_domain(c.div_a, c.div_b, div_ref(c.div_a, c.div_b))).sum()), int((~in_sqrt_domain(c.sqrt)).sum()))
