"""Shows that the counters of libnori_hip_count.so COUNT: runs exact_rcp, exact_div and exact_sqrt (Renderer.arith) over the
operands of tests/arith_cases.py::counter_cases -- a few thousand per sequence, a known number of them outside its domain --
and then over the in-domain ones alone, and prints per run the four counters and how many NaN / infinite results came back.
Two JSON lines; tests/test_gpu_arith.py compares them with what the numpy predicates say.
   NORI_HIP_LIBRARY=nori_amd/lib/libnori_hip_count.so python tools/arith_excursion_probe.py"""
import json, sys
sys.path.insert(0, ".")
import numpy as np
from nori_amd.render import Renderer
from tests import arith_cases as ac

c = ac.counter_cases()
r = Renderer(0)
for run, rcp, div, sqrt in (("mixed", c.rcp, (c.div_a, c.div_b), c.sqrt), ("inside", c.inside["rcp"], c.inside["div"], c.inside["sqrt"])):
    r.excursions(reset=True)
    out = {"rcp": r.arith("rcp", rcp), "div": r.arith("div", *div), "sqrt": r.arith("sqrt", sqrt)}
    ex = r.excursions()
    print(json.dumps({"run": run, "rcp_out_of_domain": ex[0], "div_out_of_domain": ex[1], "sqrt_out_of_domain": ex[2], "nan_or_infinite": ex[3],
                      "operands": {k: int(v.size) for k, v in out.items()},
                      "nonfinite_returned": {k: int((~np.isfinite(v)).sum()) for k, v in out.items()}}), flush=True)
r.close()
