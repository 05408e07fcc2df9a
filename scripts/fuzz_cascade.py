"""Development: random cascaded stage lists (k_cascade) against the CPU oracle — the generator of
tests/test_gpu_cascade.py::test_cascade_fuzz_against_oracle, more shapes.  usage: fuzz_cascade.py [n_shapes] [seed]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quadrs_amd as Q
from util import fuzz_cascade_shapes
from oracle import oracle as O        # the checker (test infrastructure), as in tests/conftest.py
O.lib()

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
cov, obs = {}, {}
checked, bad = fuzz_cascade_shapes(Q, n, seed, O, log=lambda m: print(m, flush=True), cov=cov, observed=obs)
print(f"checked {checked} shapes, mismatching: {len(bad)}; FIR classes {sorted(cov['cls1'])} / {sorted(cov['cls2'])}, "
      f"halved sub-tiles {sum(1 for m, s in cov['M'] if m and m < s)}, failing tails {cov['short']}, "
      f"norms bit-exact {obs['exact']}/{obs['bins']}, worst {obs['worst_ulp']:.2f} ulp")
sys.exit(1 if bad else 0)
