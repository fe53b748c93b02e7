"""What the committee surrogate (``Optimizer(surrogate="committee")``) costs on the device.

    python scripts/committee_probe.py kernels [--reps 20] [--warmup 3]
    python scripts/committee_probe.py tell [--rounds 3]

``kernels``: HIP-event milliseconds, median of ``--reps`` after ``--warmup``.
``mpo_gp_committee_score`` (EI, top-5, no rows out) over E = 4 experts of 512 rows, d = 10, at
m = 1e4 and 1e6 candidates, interleaved with the E plain ``mpo_gp_acq_score`` calls it contains
(mu / sd rows only): the committee call's time over their sum is what the folds, the finish and the
merge add.  Then ``mpo_gp_committee_grad`` (batch 15) against E calls of ``mpo_gp_acq_grad``.

``tell``: refit + proposal seconds of ONE batch ``tell`` of n points (d = 5, 10 000 candidates,
``acq_func="EI"``): at n = 512, 1024 and 2048 ``surrogate="exact"`` against ``"committee"`` with
``expert_size`` 256 and 512; at n = 4096 and 8192 the committee alone.  All arms of one n are
interleaved in one process, ``--rounds`` each after a warm-up round; the split into fit, prepare,
score and polish is ``optimizer.STATS``'s.  Nothing here says anything about search quality.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd import _lib  # noqa: E402
from mpi_opt_amd import optimizer as OPT  # noqa: E402


def med(v):
    return float(np.median(v))


def event_ms(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def kernels(a):
    import torch

    from mpi_opt_amd.gp import DeviceCommittee, DeviceGP
    from oracle.gp_ei import synthetic_problem

    L = _lib.lib()
    ref = ctypes.byref
    s = _lib.stream_handle()
    n, d, E = 2048, 10, 4
    X, y = synthetic_problem(n, d, seed=0)
    ls = 0.45 + 0.11 * (np.arange(d) % 5)
    norm = (float(np.mean(y)), float(np.std(y)))
    com = DeviceCommittee([DeviceGP(X[e::E], y[e::E], 1.3, ls, 0.05, device="cuda:0", norm=norm) for e in range(E)])
    y_opt = float(np.min(y))
    for m in (10_000, 1_000_000):
        c = torch.rand(m, d, dtype=torch.float64, device="cuda:0")
        need = L.mpo_gp_committee_ws_bytes(com.models, E, m, 5)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        wsp = torch.empty(L.mpo_gp_score_ws_bytes(ref(com.experts[0].model), m, 0), dtype=torch.uint8, device="cuda:0")
        mu, sd = torch.empty(m, dtype=torch.float64, device="cuda:0"), torch.empty(m, dtype=torch.float64, device="cuda:0")
        tki, tkv = torch.empty(3, 5, dtype=torch.int64, device="cuda:0"), torch.empty(3, 5, dtype=torch.float64, device="cuda:0")

        def committee():
            _lib.check(L.mpo_gp_committee_score(com.models, E, c.data_ptr(), m, y_opt, 0.01, 1.96, 1, None, None, None, 5,
                                                tki.data_ptr(), tkv.data_ptr(), ws.data_ptr(), need, s))

        def plain():
            for g in com.experts:
                _lib.check(L.mpo_gp_acq_score(ref(g.model), c.data_ptr(), m, 0.0, 0.0, 0.0, 1, mu.data_ptr(), sd.data_ptr(),
                                              None, 0, None, None, wsp.data_ptr(), wsp.numel(), s))

        t = {"committee": [], "plain": []}
        for fn in (committee, plain):
            event_ms(fn, 0, a.warmup)
        for _ in range(a.reps):                        # interleaved: one of each per round
            t["committee"] += event_ms(committee, 1, 0)
            t["plain"] += event_ms(plain, 1, 0)
        print(f"score E={E} x n=512 d={d} m={m} (workspace {need / 2 ** 20:.1f} MiB): committee {med(t['committee']):.4f} ms "
              f"[{min(t['committee']):.4f}, {max(t['committee']):.4f}]; {E} plain mu/sd calls {med(t['plain']):.4f} ms "
              f"[{min(t['plain']):.4f}, {max(t['plain']):.4f}]; committee / plain = "
              f"{med(t['committee']) / med(t['plain']):.4f}", flush=True)
    B = 15
    x = torch.rand(B, d, dtype=torch.float64, device="cuda:0")
    acq = torch.ones(B, dtype=torch.int32, device="cuda:0")
    f, g = torch.empty(B, dtype=torch.float64, device="cuda:0"), torch.empty(B, d, dtype=torch.float64, device="cuda:0")

    def committee_grad():
        _lib.check(L.mpo_gp_committee_grad(com.models, E, x.data_ptr(), B, acq.data_ptr(), y_opt, 0.01, 1.96,
                                           f.data_ptr(), g.data_ptr(), s))

    def plain_grad():
        for e in com.experts:
            _lib.check(L.mpo_gp_acq_grad(ref(e.model), x.data_ptr(), B, acq.data_ptr(), y_opt, 0.01, 1.96, f.data_ptr(),
                                         g.data_ptr(), s))

    t = {"committee": [], "plain": []}
    for fn in (committee_grad, plain_grad):
        event_ms(fn, 0, a.warmup)
    for _ in range(a.reps):
        t["committee"] += event_ms(committee_grad, 1, 0)
        t["plain"] += event_ms(plain_grad, 1, 0)
    print(f"grad E={E} x n=512 batch={B} [{com.grad_path} waves]: mpo_gp_committee_grad {med(t['committee']) * 1e3:.1f} us "
          f"[{min(t['committee']) * 1e3:.1f}, {max(t['committee']) * 1e3:.1f}]; {E} mpo_gp_acq_grad calls "
          f"{med(t['plain']) * 1e3:.1f} us [{min(t['plain']) * 1e3:.1f}, {max(t['plain']) * 1e3:.1f}]; ratio "
          f"{med(t['committee']) / med(t['plain']):.3f}", flush=True)


def objective(X, rng):
    X = np.asarray(X)
    return ((X[:, 0] - 0.3) ** 2 + 0.5 * (X[:, 1] - 0.7) ** 2 + 0.2 * np.sin(6 * X[:, 2]) * X[:, 3] + 0.1 * X[:, 4]
            + 0.05 * rng.randn(len(X)))


def tell(a):
    import torch

    from mpi_opt_amd.optimizer import Optimizer

    space = [(0.0, 1.0)] * 5
    keys = ("refit_s", "prepare_s", "score_s", "polish_s")
    for n in (512, 1024, 2048, 4096, 8192):
        rng = np.random.RandomState(n)
        X = rng.uniform(size=(n, 5))
        y = objective(X, rng)
        X, y = [list(map(float, r)) for r in X], [float(v) for v in y]
        arms = {"exact": {}} if n <= 2048 else {}
        arms.update({f"committee/{s}": dict(surrogate="committee", expert_size=s) for s in (256, 512) if n > s})
        secs = {k: [] for k in arms}
        split = {k: {q: [] for q in keys} for k in arms}
        for rnd in range(a.rounds + 1):                # round 0 warms every arm up and is dropped
            for arm, kw in arms.items():
                opt = Optimizer(space, acq_func="EI", random_state=1, n_initial_points=10, device="cuda:0",
                                acq_optimizer_kwargs={"n_points": 10000}, **kw)
                OPT.reset_stats()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.tell(X, y)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rnd:
                    secs[arm].append(dt)
                    for q in keys:
                        split[arm][q].append(OPT.STATS[q])
        for arm in arms:
            E = "" if arm == "exact" else f" (E = {-(-n // int(arm.split('/')[1]))})"
            print(f"tell n={n} d=5, 10000 candidates, {arm}{E}: {med(secs[arm]) * 1e3:.1f} ms [{min(secs[arm]) * 1e3:.1f}, "
                  f"{max(secs[arm]) * 1e3:.1f}]; " + ", ".join(f"{q[:-2]} {med(split[arm][q]) * 1e3:.1f} ms" for q in keys),
                  flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernels", "tell"])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()
    {"kernels": kernels, "tell": tell}[args.mode](args)
