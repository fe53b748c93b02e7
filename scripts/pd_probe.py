"""What the objective report's partial dependence costs on the device.

    python scripts/pd_probe.py [--rounds 3] [--large-rounds 1] [--sizes flagship,large] [--fused-only]

At the flagship report (n = 200, d = 10, S = 250, G = 40: 10 + 45 tasks) and one large one
(n = 1024, d = 32, S = 250, G = 40: 32 + 496 tasks) it times, with HIP events after a warm-up,

* ``fused``: the ONE ``mpo_gp_partial_dependence`` call over all tasks, repeated inside the timed
  window until the window is at least 0.2 s;
* ``rows``: the path that existed before it, on the same model in the same process, the two
  alternating: every task's rows (cells x S, the samples with the spans overwritten) are
  materialised on the device task by task and scored by ``DeviceGP.score`` for mu only, then
  averaged over the samples.

It prints both times per round, their medians, the largest difference of the two results, the
fused call's Matern evaluations per second and what share of the fp64 VALU issue rate DESIGN
§3.1 measured that is (``v_fma / v_mul / v_add_f64`` at 6.5 cycles per wave instruction on 1024
SIMDs at 2.4 GHz, the ~47 TF/s figure), at the 39 fp64 instructions per evaluation of the
kernel's inner loop (counted in its ISA: 14 the square root, 23 the polynomial and the
exponential, 2 the sums; the 14 moves and selects beside them are not counted).  Compares,
``v_ldexp`` and converts are among the 39 and may issue faster than an fma, so the share is an
upper estimate of the issue time and can pass 100 %.  ``--fused-only`` runs the fused call alone
a few times: the run to put under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse
import ctypes
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd import _lib  # noqa: E402
from mpi_opt_amd.gp import DeviceGP, pd_table  # noqa: E402

SIZES = {"flagship": (200, 10, 250, 40), "large": (1024, 32, 250, 40)}
FP64_PER_EVAL = 39
VALU_WAVE_INSTR_PER_S = 1024 * 2.4e9 / 6.5


def tasks_of(d, g):
    lin = np.linspace(0.0, 1.0, g)
    return [(i, lin) for i in range(d)] + [(i, lin, j, lin) for i in range(d) for j in range(i + 1, d)]


def model(n, d):
    from oracle.gp_ei import synthetic_problem

    X, y = synthetic_problem(n, d, seed=n + d)
    return DeviceGP(X, y, 1.3, 0.45 + 0.11 * (np.arange(d) % 5), 0.02, device="cuda:0")


class Fused:
    def __init__(self, g, smp, tasks):
        import torch

        self.g, self.L = g, _lib.lib()
        self.table, grid, self.shapes, total = pd_table(tasks)
        self.T = len(tasks)
        self.s = g.as_candidates(smp)
        self.need = self.L.mpo_gp_pd_ws_bytes(ctypes.byref(g.model), self.s.shape[0], self.table, self.T)
        assert self.need > 0
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda:0")
        self.grid = torch.from_numpy(grid).cuda()
        self.out = torch.empty(total, dtype=torch.float64, device="cuda:0")
        self.stream = _lib.stream_handle()

    def __call__(self):
        rc = self.L.mpo_gp_partial_dependence(ctypes.byref(self.g.model), self.s.data_ptr(), self.s.shape[0],
                                              self.table, self.T, self.grid.data_ptr(), self.out.data_ptr(),
                                              self.ws.data_ptr(), self.need, self.stream)
        _lib.check(rc, "mpo_gp_partial_dependence")


class Rows:
    """The materialised path: per task, rows [cells * S][d] on the device, DeviceGP.score for mu."""

    def __init__(self, g, smp, tasks):
        import torch

        self.g, self.tasks = g, tasks
        self.s = g.as_candidates(smp)
        self.grids = [[torch.from_numpy(np.asarray(t[q + 1], dtype=np.float64).reshape(len(t[q + 1]), -1)).cuda()
                       for q in range(0, len(t), 2)] for t in tasks]
        self.total = sum(int(np.prod([len(t[q + 1]) for q in range(0, len(t), 2)])) for t in tasks)
        self.out = torch.empty(self.total, dtype=torch.float64, device="cuda:0")
        self.peak_rows = 0

    def __call__(self):
        S, d = self.s.shape
        off = 0
        for t, gr in zip(self.tasks, self.grids):
            ga = gr[0].shape[0]
            gb = gr[1].shape[0] if len(gr) == 2 else 1
            rows = self.s.expand(ga, gb, S, d).contiguous()
            rows[:, :, :, t[0]:t[0] + gr[0].shape[1]] = gr[0][:, None, None, :]
            if len(gr) == 2:
                rows[:, :, :, t[2]:t[2] + gr[1].shape[1]] = gr[1][None, :, None, :]
            rows = rows.view(ga * gb * S, d)
            self.peak_rows = max(self.peak_rows, rows.shape[0])
            mu = self.g.score(rows, 0.0, acqs=("EI",), k=0, want_mu_sd=True, want_values=False)["mu"]
            self.out[off:off + ga * gb] = mu.view(ga * gb, S).mean(dim=1)
            off += ga * gb


def timed(fn, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--large-rounds", type=int, default=1)
    ap.add_argument("--sizes", default="flagship,large")
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    for name in a.sizes.split(","):
        n, d, S, G = SIZES[name]
        g = model(n, d)
        tasks = tasks_of(d, G)
        smp = np.random.RandomState(1).uniform(size=(S, d))
        fused = Fused(g, smp, tasks)
        evals = sum(int(np.prod(s)) for s in fused.shapes) * S * n
        rows_total = sum(int(np.prod(s)) for s in fused.shapes) * S
        print(f"== {name}: n={n} d={d} S={S} G={G}, {len(tasks)} tasks, {evals:.3e} Matern evaluations, "
              f"{rows_total:.3e} rows ({rows_total * d * 8 / 2 ** 30:.2f} GiB if all were materialised at once); "
              f"fused workspace {fused.need / 2 ** 20:.1f} MiB", flush=True)
        fused()
        torch.cuda.synchronize()
        one = timed(fused, 1)
        reps = max(1, int(math.ceil(200.0 / one)))
        if a.fused_only:
            for _ in range(3):
                fused()
            torch.cuda.synchronize()
            print(f"fused-only: 5 calls made (first timed call {one:.3f} ms)")
            continue
        base = Rows(g, smp, tasks)
        base()
        torch.cuda.synchronize()
        diff = float((fused.out - base.out).abs().max())
        print(f"largest |fused - rows| over all cells: {diff:.3e} (y_std {g.y_std:.3f}); the largest task holds "
              f"{base.peak_rows} rows ({base.peak_rows * d * 8 / 2 ** 20:.0f} MiB)", flush=True)
        reps_rows = max(1, int(math.ceil(200.0 / timed(base, 1))))
        tf, tr = [], []
        for r in range(a.rounds if name == "flagship" else a.large_rounds):
            tf.append(timed(fused, reps))
            tr.append(timed(base, reps_rows))
            print(f"round {r}: fused {tf[-1]:.3f} ms ({reps} calls in the window), rows {tr[-1]:.3f} ms "
                  f"({reps_rows} passes)", flush=True)
        mf, mr = float(np.median(tf)), float(np.median(tr))
        rate = evals / (mf * 1e-3)
        share = rate * FP64_PER_EVAL / 64 / VALU_WAVE_INSTR_PER_S
        print(f"{name}: fused median {mf:.3f} ms (min {min(tf):.3f}), rows median {mr:.3f} ms (min {min(tr):.3f}): "
              f"rows / fused = {mr / mf:.2f}")
        bound = "VALU issue" if share >= 0.5 else "not VALU issue (latency or occupancy: under half the issue rate)"
        print(f"{name}: {rate:.3e} Matern evaluations / s = {share:.1%} of the fp64 VALU issue rate "
              f"({FP64_PER_EVAL} fp64 instructions per evaluation against 6.5 cycles per wave instruction); "
              f"bound: {bound}; memory is not it (the call's workspace is {fused.need / 2 ** 20:.1f} MiB)", flush=True)


if __name__ == "__main__":
    main()
