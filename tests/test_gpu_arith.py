"""The device's own arithmetic where it runs: exact_rcp / exact_div / exact_sqrt (rt_types.h), slab_rcp (rt_trace.h) and the
specified sin / cos / log / exp (rt_math.h), evaluated by the product library (Renderer.arith -> nori_hip_debug_arith) and held
bit pattern by bit pattern to IEEE arithmetic done on the CPU.  Every parity claim of the suite rests on these few
instruction sequences; they exist only in the device compilation, so nothing else tests them.

Operands, references and domains: tests/arith_cases.py (checked by tests/test_arith_cases_cpu.py).  Inside the stated domains
ZERO bit patterns may differ, signs of zero included; outside them nothing is asserted, except for slab_rcp, which is defined
everywhere.  exact_div's one stated departure from IEEE -- -0 / b is +0 for b > 0 -- is asserted as stated.

Measured on an MI355X when this file was written: 0 mismatches for every operation (52.4 M reciprocals, 17.7 M roots, 16.8 M
quotients in either form, 0.5 M slab reciprocals, 18.5 M sines and cosines, 2.1 M logarithms and exponentials); -0 / b came back
+0 for b > 0 and the other three sign pairs as IEEE has them; of the 2016 quotients just outside the domain that round to
FLT_MAX (arith_cases.div_outside_top) 1008 came back NaN.

What the tests catch, from one run against a library built with two edits to rt_types.h: without the Newton step of
exact_rcp_raw 5.6 M of the 52.4 M reciprocals differ (897 675 in each exhaustive binade), 39 573 slab reciprocals, and of the
quotients ONLY class (c) -- 8116 of its 1.29 M pairs: the other 15.5 M pairs, the mantissa patterns included, still pass;
without the neighbour correction of exact_sqrt 2.5 M of the 16.8 M roots of [1, 4) differ."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import arith_cases as ac
from tests.arith_cases import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    from nori_amd.render import Renderer
    r = Renderer(0)
    yield r
    r.close()


class Tally:
    """bit mismatches of one operation over many calls: how many, in which sets, and the first few in hexadecimal"""

    def __init__(self, op):
        self.op, self.n, self.bad, self.per_label, self.first = op, 0, 0, {}, []

    def add(self, label, operands, want, got):
        wrong = bits(want) != bits(got)
        k = int(wrong.sum())
        self.n += want.size
        self.bad += k
        self.per_label[label] = self.per_label.get(label, 0) + k
        for i in np.flatnonzero(wrong)[:max(0, 8 - len(self.first))]:
            self.first.append(f"{label}: " + " , ".join(f"{int(bits(o)[i]):#010x}" for o in operands) + f" -> expected {int(bits(want)[i]):#010x} got {int(bits(got)[i]):#010x}")

    def check(self):
        print(f"[arith] {self.op}: {self.n} operands, {self.bad} bit mismatches", {k: v for k, v in self.per_label.items() if v} or "")
        assert self.bad == 0, f"{self.op}: {self.bad} of {self.n} results differ from the reference; per set {self.per_label}; first: " + " | ".join(self.first)


def _run(dev, op, label, tally, want_fn, *operands):
    """op over the operands in calls of at most ac.CHUNK elements"""
    for part in ac.chunks(*operands):
        assert part[0].size <= ac.CHUNK
        tally.add(label, part, want_fn(*part), dev.arith(op, *part))


def test_exact_rcp_is_the_ieee_reciprocal(dev):
    """All 2^23 mantissas at 2^0, 2^-126 and 2^125 (the middle and the ends of the domain), both signs; 4096 at every other
    exponent: 52 M operands, against float32(1) / x."""
    t = Tally("rcp")
    for label, x in ac.rcp_chunks():
        t.add(label, (x,), ac.rcp_ref(x), dev.arith("rcp", x))
    t.check()


@pytest.mark.parametrize("op", ["div", "div_shared"])
def test_exact_div_is_the_ieee_quotient(dev, op):
    """2^24 pairs inside the stated domain, in the classes of tests/arith_cases.py (exponents over the WHOLE domain, mantissa
    patterns, quotients 2^-24 ulp from a midpoint, zero numerators, exact integer quotients, the domain's edges), against a / b
    in float32 -- with the one stated exception for a zero numerator (rt_types.h): -0 / b, b > 0, is +0.  `div_shared` is the
    form f3 / float uses: one reciprocal, three quotients."""
    d = ac.div_cases()
    t = Tally(op)
    zero = []
    for a, b, cls in ac.chunks(d.a, d.b, d.cls):
        got = dev.arith(op, a, b)
        want = ac.div_contract(a, b)
        for c, name in enumerate(ac.DIV_CLASSES):
            m = cls == c
            if m.any():
                t.add(name, (a[m], b[m]), want[m], got[m])
        z = cls == 3
        zero.append(np.stack([bits(a[z]) >> 31, bits(b[z]) >> 31, bits(got[z])], 1))
    zero = np.concatenate(zero)
    returned = {f"{'-+'[sa == 0]}0 / {'-+'[sb == 0]}b": sorted(f"{int(v):#010x}" for v in np.unique(zero[(zero[:, 0] == sa) & (zero[:, 1] == sb), 2]))
                for sa in (0, 1) for sb in (0, 1)}
    print(f"[arith] {op}: zero numerators returned", returned)
    t.check()
    # class (d), exactly as the header states it
    assert returned == {"+0 / +b": ["0x00000000"], "+0 / -b": ["0x80000000"], "-0 / +b": ["0x00000000"], "-0 / -b": ["0x00000000"]}


def test_exact_sqrt_is_the_ieee_root(dev):
    """Every float of [1, 4) (inside the domain only the mantissa and the exponent's parity matter: exhaustive over what can
    differ), 4096 mantissas at every exponent from 2^-104 up, the perfect squares below 2^24, +-0, +inf, 2^-104: against np.sqrt."""
    t = Tally("sqrt")
    for label, x in ac.sqrt_cases():
        _run(dev, "sqrt", label, t, ac.sqrt_ref, x)
    t.check()


def test_slab_rcp_is_the_clamped_reciprocal(dev):
    """slab_rcp(d) = copysign(min(|1 / d|, 2^60), d) for every d below 2^126: zeros and denormals of both signs included."""
    t = Tally("slab_rcp")
    _run(dev, "slab_rcp", "every exponent, zeros, denormals, 2^-60", t, ac.slab_ref, ac.slab_cases())
    t.check()


@pytest.mark.parametrize("op", ["sin", "cos", "log", "exp"])
def test_specified_transcendentals_on_the_device(dev, op):
    """det_sincosf / det_logf / det_expf as compiled for gfx950 equal the oracle's implementation of the same specification
    (binary64, no FMA, one rounding) bit for bit on every argument set -- the quadrant switches and the cancellation end of log
    exhaustively --, and the correctly rounded value on the ranges the CPU compilation is held to it."""
    from tests.backends import Oracle
    t, tc = Tally(op + " vs oracle"), Tally(op + " vs correctly rounded")
    for label, x, cr in ac.libm_cases(op):
        want = Oracle.libm(op, x)
        for (xs, ws) in ac.chunks(x, want):
            got = dev.arith(op, xs)
            t.add(label, (xs,), ws, got)
            if cr:
                tc.add(label, (xs,), ac.correctly_rounded(op, xs), got)
            if op == "exp" and label == "edges":
                tc.add(label, (xs,), ac.EXP_EDGES_EXPECTED, got)
    t.check()
    tc.check()


def test_arith_rejects_what_it_cannot_evaluate(dev):
    from nori_amd._capi import NoriError
    with pytest.raises(ValueError):
        dev.arith("div", np.ones(4, np.float32))
    with pytest.raises(ValueError):
        dev.arith("rcp", np.ones(4, np.float32), np.ones(4, np.float32))
    with pytest.raises(NoriError):
        dev._check(dev._lib.nori_hip_debug_arith(dev._h, 99, None, None, 0, None), "debug_arith")
    assert dev.arith("sqrt", np.zeros(0, np.float32)).size == 0
    x = np.float32([[4.0, 9.0, 0.25]])      # one thread group, not full; the shape comes back
    assert np.array_equal(dev.arith("sqrt", x), np.float32([[2.0, 3.0, 0.5]]))


def test_the_excursion_counters_count():
    """The two `stays inside its verified domain` tests assert that four counters of libnori_hip_count.so are zero -- which a
    condition that never fires would pass too.  Here the same library evaluates rcp, div and sqrt over a few thousand operands of
    which a known number lie outside each domain (a factor 4 away from its border at least): counters 0 .. 2 are exactly the
    numbers the numpy predicates of tests/arith_cases.py give, counter 3 the number of NaN / infinite results the same calls
    returned; in-domain operands alone leave four zeros.  Any of the library's conditions replaced by `false` changes a count
    asserted here (every expected count is non-zero, and so is each call's share of counter 3).  Fresh process: the library is
    chosen when it is loaded."""
    lib = os.path.join(ROOT, "nori_amd", "lib", "libnori_hip_count.so")
    assert os.path.exists(lib), "libnori_hip_count.so missing: __graft_entry__.build() makes it"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "arith_excursion_probe.py")], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, NORI_HIP_LIBRARY=lib), timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    rows = {r["run"]: r for r in (json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{"))}
    assert sorted(rows) == ["inside", "mixed"]
    for row in rows.values():
        print("[excursions]", row)
    c = ac.counter_cases()
    want = ac.counter_expectation(c)
    mixed, inside = rows["mixed"], rows["inside"]
    assert mixed["operands"] == {"rcp": c.rcp.size, "div": c.div_a.size, "sqrt": c.sqrt.size}
    assert min(want) > 0
    assert (mixed["rcp_out_of_domain"], mixed["div_out_of_domain"], mixed["sqrt_out_of_domain"]) == want
    nf = mixed["nonfinite_returned"]
    assert nf["rcp"] > 0 and nf["div"] > 0      # both conditions on results have something to count
    assert mixed["nan_or_infinite"] == nf["rcp"] + nf["div"]      # exact_sqrt has no such condition: sqrt(+inf) is a result, not an excursion
    assert (inside["rcp_out_of_domain"], inside["div_out_of_domain"], inside["sqrt_out_of_domain"], inside["nan_or_infinite"]) == (0, 0, 0, 0)
    assert inside["nonfinite_returned"]["rcp"] == 0 and inside["nonfinite_returned"]["div"] == 0
