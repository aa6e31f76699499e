"""ll bits of two builds of the library on the same random inputs (run once
per build: python tools/ab_bits_libs.py <out.npy> [batch]; NEMO_LIBRARY picks
the build; batch defaults to 257, which splits a C3 evaluation over two
blocks -- past 1024, every family's block slots, one block holds a whole
evaluation and the in-kernel sum of its partials runs), for changes that
must not move a bit: every fact_kernel value on C3
and C2 (uncapped, and capped at 5 so that the lookup-table kernels 9 / 15
resolve) and on W128 (64 < S <= 128, where 18 / 19 resolve), auto with the
fast kernels included.  A call the library refuses counts as REFUSED."""
import sys
sys.path.insert(0, "nem-mcmc-optimization_amd")
import numpy as np  # noqa: E402
from scipy.special import expit  # noqa: E402

from nemo import generator  # noqa: E402
from nemo.engine import Engine  # noqa: E402

REFUSED = -1.0e300
B = int(sys.argv[2]) if len(sys.argv) > 2 else 257
out = []
for cfg, caps in (("C3", (0, 5)), ("C2", (0, 5)), ("W128", (0,))):
    m = generator.config_nem(cfg)
    eng = Engine.for_nem(m)
    S = m.num_s
    rng = np.random.default_rng(11)
    pos = np.array([rng.permutation(S) for _ in range(B)], dtype=np.int32)
    w = expit(rng.uniform(-3, 3, (B, S, S)))
    for cap in caps:
        for exact, fk in [(1, 0)] + [(0, v) for v in range(21)]:
            eng.set_option("exact", exact)
            eng.set_option("fact_kernel", fk)
            try:
                ll = eng.score(pos, w, cap=cap)
                took = eng.score_kernel(cap=cap)[0]
            except RuntimeError:
                ll, took = np.full(B, REFUSED), -1
            print(cfg, "cap", cap, "exact", exact, "fact_kernel", fk, "->", took, flush=True)
            out.append(np.append(ll, took))
    eng.close()
np.save(sys.argv[1], np.concatenate(out))
