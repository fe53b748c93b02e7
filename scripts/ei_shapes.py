"""Time one resident GP scoring pass (1M candidates, d = 10, top-5 EI) at other
observation counts than the flagship's: ``python scripts/ei_shapes.py 48 600 1232``.
MPO_LIB_AB selects another build's libmpo.so (scripts/ab_lib.py)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scripts.ab_lib  # noqa: E402,F401 -- MPO_LIB_AB: another build's libmpo.so (same-box A/B)
from mpi_opt_amd import synthetic  # noqa: E402
from mpi_opt_amd.gp import DeviceGP  # noqa: E402

ls = np.array([16.2, 1.91, 1.65, 9.84, 1.84, 2.94, 2.45, 9.09, 8.13, 1.94])
cand = torch.from_numpy(synthetic.gp_candidates(1_000_000, 10, seed=1)).cuda()
for n in [int(v) for v in sys.argv[1:]] or [48, 200, 600, 1232]:
    X, y = synthetic.gp_problem(n, 10, 0)
    g = DeviceGP(X, y, 17.4955, ls, 0.0465)
    reps = 5 if n <= 600 else 2
    ts = []
    for rnd in range(5):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.score(cand, float(y.min()), k=5)
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            ts.append(e0.elapsed_time(e1) / reps)
    print("n=%-5d median %.3f ms  min %.3f ms  max %.3f ms" % (n, np.median(ts), np.min(ts), np.max(ts)), flush=True)
