"""One long seeded walk over the cells of tests/sequence_cases.py on the process-wide engine — the open-ended form of
tests/test_gpu_sequences.py::test_walks_on_the_process_engine: every operator family at the sizes S, L and sometimes G (which
re-creates the engine), refusing calls and pokes at the sticky settings in between, every result compared bit for bit with what a
newly created engine gave at the start.  Prints the seed and the index of the first call that differs (and stops there).
usage: python tools/sequence_fuzz.py [calls] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch                                    # (before the library: the order tests/conftest.py keeps)
    torch.cuda.is_available() and torch.cuda.init()
except ImportError:
    pass
import pyitd_amd as P
import sequence_cases as sc
from test_gpu_sequences import walk

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 500
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
steps = sc.walk_schedule(seed, walks=1, calls=max(calls, 4 * len(sc.NAMES) + 80))[0][:calls]
t0 = time.time()
fresh = {}
for name, size in sorted({(s["cell"], s["size"]) for s in steps}):
    sc.fresh_engines(P)
    cell = sc.CELLS[name]
    fresh[name, size] = cell.run(P, cell.inputs(size))
    with np.errstate(all="ignore"):
        cell.check(cell.inputs(size), fresh[name, size], P)
sc.fresh_engines(P)
t1 = time.time()
first, msg = walk(P, lambda c, s: fresh[c, s], steps, "seed %d" % seed)
kinds = {k: sum(1 for s in steps if s[k] is not None) for k in ("refusal", "solver", "fuse_min")}
print("seed %d: %d calls over %d cells (%d at G, %d refusing calls, %d solver and %d threshold pokes in front), %d fresh results in %.1f s, the walk in %.1f s" % (
    seed, len(steps), len({s["cell"] for s in steps}), sum(s["size"] == "G" for s in steps), kinds["refusal"], kinds["solver"], kinds["fuse_min"],
    len(fresh), t1 - t0, time.time() - t1))
if first is None:
    print("seed %d: no call differs from a fresh engine" % seed)
    sys.exit(0)
print("seed %d: FIRST DIFFERING CALL %d: %s" % (seed, first, msg[:600]))
sys.exit(1)
