"""Write tests/golden/i8l_walk_parent.npz: ll of fact_kernel 10 on the seeded
inputs of tests/walk_sched_inputs.py, one array of seven doubles per shape and
cap.  Run ONCE on an MI355X with the library built from the commit before the
two-tile walk's software pipeline (NEMO_LIBRARY picks the build):

    NEMO_LIBRARY=<parent build>/libnemo.so python tools/make_walk_golden.py [out.npz]

tests/test_gpu_walk_sched.py holds kernels 10, 17 and 20 to these bits.  The
file also names the build id that wrote it.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nem-mcmc-optimization_amd", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import numpy as np  # noqa: E402

import walk_sched_inputs as wi  # noqa: E402
from nemo import _lib  # noqa: E402
from nemo.engine import Engine  # noqa: E402

out = {}
for s, e in wi.CASES:
    m, _, pos, w01 = wi.inputs(s, e)
    eng = Engine.for_nem(m)
    try:
        eng.set_option("exact", 0)
        eng.set_option("fact_kernel", 10)
        for cap in wi.CAPS:
            assert eng.score_kernel(cap)[0] == 10
            out[wi.key(s, e, cap)] = eng.score(pos, w01, cap=cap)
            print(wi.key(s, e, cap), out[wi.key(s, e, cap)], flush=True)
    finally:
        eng.close()
out["build_id"] = np.array(_lib.build_id())
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", wi.GOLDEN)
np.savez(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
