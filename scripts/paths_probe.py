"""Pathwise Thompson ask batches against the joint ones, and the device time of the two
entry points they draw through.

    python scripts/paths_probe.py batches [--ask-n 256] [--rounds 7]
    python scripts/paths_probe.py kernels [--sizes 256:2048:256:2048,...] [--reps 20] [--warmup 3]
    python scripts/paths_probe.py polish [--ask-n 256] [--rounds 7] [--grad-sizes 256:2048:256,...]

``batches``: a lone ``ask(N)`` after 256 tells (the setup of scripts/thompson_probe.py), four
arms interleaved in rounds in one process -- ``joint`` at n_ts = 2048, ``paths`` at 2048, at
10 000 and at 1 000 000 with ``candidates="device"`` -- median and min-max of the seconds per
batch and the host-clock split of the step (candidates, draws on the host, prepare, eval,
dedupe; the joint arm has candidates, sample and dedupe only).

``polish``: the same setup with two arms, ``paths`` at 10 000 candidates without and with
``ts_polish``: seconds per batch, the split (``polish_s`` among it), the rounds of the lockstep
L-BFGS-B, the collisions, how many draws kept their polished point, and (from one further,
traced and untimed batch) the decrease of each draw's value in units of y_std sqrt(amp).  Then
HIP-event milliseconds of one ``mpo_gp_paths_grad`` at (n, F, batch), median of ``--reps``
after ``--warmup``.

``kernels``: HIP-event milliseconds of ``mpo_gp_paths_prepare`` and ``mpo_gp_paths_eval``
(argmin and minval, no sample rows) at (n, m, s, F), median of ``--reps`` after ``--warmup``,
the eval as a fraction of the nominal 78.6 TFLOP/s over 2 m s (Fp + np16) MFMA FLOP, and
``mpo_gp_sample`` at (256, 2048, 256) alternating with every shape.
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
from scripts.thompson_probe import stats, told_optimizer  # noqa: E402

NOMINAL_TFLOPS = 78.6


BATCH_ARMS = {"joint 2048": ({"n_ts_points": 2048}, {}),
              "paths 2048": ({"ts_sampler": "paths", "n_ts_points": 2048}, {}),
              "paths 10000": ({"ts_sampler": "paths", "n_ts_points": 10000}, {}),
              "paths 1000000 device": ({"ts_sampler": "paths", "n_ts_points": 1000000}, {"candidates": "device"})}
POLISH_ARMS = {"paths 10000": ({"ts_sampler": "paths", "n_ts_points": 10000}, {}),
               "paths 10000 polish": ({"ts_sampler": "paths", "n_ts_points": 10000, "ts_polish": True}, {})}


def batches(a, arms=BATCH_ARMS):
    import torch

    secs = {k: [] for k in arms}
    split = {k: {} for k in arms}
    step = OPT._thompson_step
    step_start = []

    def timed_step(opt, r):
        torch.cuda.synchronize()
        step_start.append(time.perf_counter())
        out = step(opt, r)
        timed_step.times = dict(opt.thompson_times)
        timed_step.times["collisions"] = getattr(opt, "thompson_collisions", float("nan"))   # a count, not seconds
        if opt.acq_optimizer_kwargs.get("ts_polish", False):                                 # counts too
            timed_step.times["polish_rounds"] = opt.thompson_polish_rounds
            timed_step.times["polished_kept"] = opt.thompson_polished
        return out

    OPT._thompson_step = timed_step
    for rnd in range(a.rounds + 1):                # round 0 warms every arm up and is dropped
        for name, (aok, kw) in arms.items():
            opt = told_optimizer(acq_optimizer_kwargs=dict(aok), **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X = opt.ask(a.ask_n, "thompson")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                secs[name].append(dt)
                split[name].setdefault("copy_and_fit_s", []).append(step_start[-1] - t0)
                for k, v in timed_step.times.items():
                    split[name].setdefault(k, []).append(v)
            print(f"round {rnd} {name}: ask({a.ask_n}) {dt:.4f} s, first point {list(X[0])}", flush=True)
    for name, v in secs.items():
        print(f"{name}: {len(v)} batches, seconds {stats(v)}")
        for k, t in split[name].items():
            print(f"    {k}: {stats(t)}")
    OPT._thompson_step = step


def polish(a):
    import torch

    from mpi_opt_amd.gp import DeviceGP
    from mpi_opt_amd.paths import draw_paths
    from oracle import gp_ei as O

    batches(a, POLISH_ARMS)
    # one traced, untimed batch: what the polish does to each draw's value
    opt = told_optimizer(acq_optimizer_kwargs=dict(POLISH_ARMS["paths 10000 polish"][0]))
    opt.trace = []
    opt.ask(a.ask_n, "thompson")
    rec = opt.batch_trace[-1]
    pol = rec["polish"]
    y = np.asarray(opt.yi)
    scale = float(np.std(y)) * np.sqrt(rec["theta"][0])
    drop = (pol["f_start"] - pol["f"]) / scale
    st = pol["stats"]
    print(f"traced batch: {sum(pol['kept'])} of {len(drop)} draws kept their polished point; decrease of the draw's "
          f"value in y_std sqrt(amp): median {np.median(drop):.4g} (min {drop.min():.4g}, max {drop.max():.4g}); "
          f"nit median {np.median(st[:, 0]):.0f} max {st[:, 0].max()}, nfev median {np.median(st[:, 1]):.0f} max "
          f"{st[:, 1].max()}, statuses {sorted(set(st[:, 2].tolist()))}", flush=True)

    # device time of one mpo_gp_paths_grad
    L, P, d = _lib.lib(), _lib.ptr, a.d
    amp, ls, noise = 2.0, np.linspace(0.5, 2.0, d), 0.05
    for n, F, B in (tuple(int(v) for v in sz.split(":")) for sz in a.grad_sizes.split(",")):
        X, yy = O.synthetic_problem(n, d, seed=n + d)
        g = DeviceGP(X, yy, amp, ls, noise)
        dev = g.device
        s = min(B, _lib.MPO_PATHS_SMAX)
        p = g.paths(*draw_paths(np.random.RandomState(3), F, d, s, n))
        x = torch.rand(B, d, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(7))
        dr = (torch.arange(B, device=dev) % s).to(torch.int32)
        f = torch.empty(B, dtype=torch.float64, device=dev)
        gr = torch.empty(B, d, dtype=torch.float64, device=dev)
        stream = _lib.stream_handle(dev)
        ms = []
        for it in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.mpo_gp_paths_grad(ctypes.byref(g.model), ctypes.byref(p.paths), P(x), P(dr), B, P(f), P(gr),
                                           stream), "mpo_gp_paths_grad")
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        print(f"mpo_gp_paths_grad n {n} F {F} batch {B} d {d}: {stats(ms)} ms over {len(ms)} launches", flush=True)


def kernels(a):
    import torch

    from mpi_opt_amd.gp import DeviceGP
    from mpi_opt_amd.paths import draw_paths
    from oracle import gp_ei as O

    L = _lib.lib()
    d = a.d
    amp, ls, noise = 2.0, np.linspace(0.5, 2.0, d), 0.05
    P = _lib.ptr

    def timed(fn, out):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))

    # the joint sampler's reference shape
    Xj, yj = O.synthetic_problem(256, d, seed=256 + d)
    gj = DeviceGP(Xj, yj, amp, ls, noise)
    Cj = gj.as_candidates(O.synthetic_candidates(2048, d, seed=7))
    Zj = torch.from_numpy(np.random.RandomState(3).standard_normal((2048, 256))).to(gj.device)
    wsj, wsjb = gj._ensure_joint_ws(2048, 256)
    amj = torch.empty(256, dtype=torch.int64, device=gj.device)
    infoj = torch.empty(1, dtype=torch.int32, device=gj.device)
    stj = _lib.stream_handle(gj.device)

    def joint():
        _lib.check(L.mpo_gp_sample(ctypes.byref(gj.model), P(Cj), 2048, P(Zj), 256, 1e-8, None, P(amj), P(infoj),
                                   P(wsj), wsjb, stj), "mpo_gp_sample")

    for n, m, s, F in (tuple(int(v) for v in sz.split(":")) for sz in a.sizes.split(",")):
        X, y = O.synthetic_problem(n, d, seed=n + d)
        g = DeviceGP(X, y, amp, ls, noise)
        dev = g.device
        C = torch.rand(m, d, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(7))
        om, ph, w, ep = (torch.from_numpy(v).to(dev) for v in draw_paths(np.random.RandomState(3), F, d, s, n))
        md = ctypes.byref(g.model)
        wsb = L.mpo_gp_paths_ws_bytes(md, F, s)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        pt = _lib.MpoGpPaths()
        st = _lib.stream_handle(dev)
        argmin = torch.empty(s, dtype=torch.int64, device=dev)
        minval = torch.empty(s, dtype=torch.float64, device=dev)

        def prepare():
            _lib.check(L.mpo_gp_paths_prepare(md, noise, P(om), P(ph), P(w), P(ep), F, s, ctypes.byref(pt), P(ws), wsb,
                                              st), "mpo_gp_paths_prepare")

        prepare()
        ewsb = L.mpo_gp_paths_eval_ws_bytes(md, ctypes.byref(pt), m, s)
        ews = torch.empty(ewsb, dtype=torch.uint8, device=dev)

        def evaluate():
            _lib.check(L.mpo_gp_paths_eval(md, ctypes.byref(pt), P(C), m, 0, s, None, P(argmin), P(minval), P(ews),
                                           ewsb, st), "mpo_gp_paths_eval")

        ms = {"prepare": [], "eval": [], "joint_sample_256_2048_256": []}
        reps = max(3, a.reps // 4) if m >= 500000 else a.reps
        for it in range(a.warmup + reps):
            for name, fn in (("prepare", prepare), ("eval", evaluate), ("joint_sample_256_2048_256", joint)):
                sink = ms[name] if it >= a.warmup else []
                timed(fn, sink)
        flop = 2.0 * m * s * (pt.Fp + g.model.np16)
        ev = float(np.median(ms["eval"]))
        print(f"n {n} m {m} s {s} F {F} d {d}, prepare ws {wsb / 2**20:.1f} MiB: " +
              ", ".join(f"{k} {stats(v)} ms" for k, v in ms.items()) +
              f"; eval {flop / 1e12:.3f} TFLOP, {flop / (ev * 1e-3) / 1e12:.1f} TFLOP/s, "
              f"{100.0 * flop / (ev * 1e-3) / 1e12 / NOMINAL_TFLOPS:.1f}% of nominal {NOMINAL_TFLOPS}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    b = sub.add_parser("batches")
    b.add_argument("--ask-n", type=int, default=256)
    b.add_argument("--rounds", type=int, default=7)
    k = sub.add_parser("kernels")
    k.add_argument("--sizes", default="256:2048:256:2048,256:10000:256:2048,256:1000000:256:2048,"
                                      "2048:1000000:256:2048")
    k.add_argument("--d", type=int, default=5)
    k.add_argument("--reps", type=int, default=20)
    k.add_argument("--warmup", type=int, default=3)
    q = sub.add_parser("polish")
    q.add_argument("--ask-n", type=int, default=256)
    q.add_argument("--rounds", type=int, default=7)
    q.add_argument("--grad-sizes", default="256:2048:256,2048:4096:1024")
    q.add_argument("--d", type=int, default=5)
    q.add_argument("--reps", type=int, default=50)
    q.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    {"batches": batches, "kernels": kernels, "polish": polish}[a.mode](a)


if __name__ == "__main__":
    main()
