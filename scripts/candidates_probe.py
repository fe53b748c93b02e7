"""The pieces of one proposal with host-drawn, device-drawn and lattice candidates
(``Optimizer(candidates=...)``): sample, host-to-device copy, score (top-k of the three
acquisitions), gather + polish, total -- host-clock milliseconds, each piece ended by a
device synchronise, median and range over ``--reps`` proposals after ``--warmup``.  The
sources alternate proposal by proposal in one process, on one fixed-theta model of
``--told`` points.  The lattice source writes L * max(1, ceil(n_points / L)) rows and its
polish holds the discrete columns still.  Also the writers' device time (HIP events) at
equal rows beside a ``torch.Tensor.fill_`` of the same tensor, the practical store yardstick.

``--loss K``: instead, K seeded proposals of ``Optimizer(acq_func="EI")`` per source on the
MNIST space after 64 told points, and the oracle's EI (oracle.gp_ei, at the fitted theta) at
the point each source finally trains -- after ``inverse_transform`` -- beside the EI at the
point its polish returned.  The difference is what the relaxation of the discrete
dimensions costs a proposal; it says nothing about search quality.

    python scripts/candidates_probe.py [--space mnist,real10,real10int2] [--n-points 1000000] [--told 200]
                                       [--source both|all|host|device|lattice] [--reps 20] [--warmup 3]
    python scripts/candidates_probe.py --loss 20 [--n-points 10000]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd.blocks import _device_topk  # noqa: E402
from mpi_opt_amd.candidates import frozen_columns, lattice_size, lattice_transformed, sample_transformed  # noqa: E402
from mpi_opt_amd.models import mnist_space  # noqa: E402
from mpi_opt_amd.optimizer import DRIVER, GPModel, Optimizer, polish_lockstep  # noqa: E402
from mpi_opt_amd.space import Integer, Real, Space  # noqa: E402

ACQS = ("EI", "LCB", "PI")
PIECES = ("sample", "copy", "score", "polish", "total")


def proposal(source, space, est, n_points, rng, dev):
    """One proposal's pieces in seconds; the candidates end up on the device either way."""
    y_opt = float(np.min(est.y))
    frozen = None
    t0 = time.perf_counter()
    if source == "lattice":
        L = lattice_size(space)
        frozen = frozen_columns(space)
        X = lattice_transformed(space, L * max(1, -(-n_points // L)), int(rng.randint(0, np.iinfo(np.int32).max)), dev)
        torch.cuda.synchronize(dev)
        t1 = t2 = time.perf_counter()
    elif source == "device":
        X = sample_transformed(space, n_points, int(rng.randint(0, np.iinfo(np.int32).max)), dev)
        torch.cuda.synchronize(dev)
        t1 = t2 = time.perf_counter()
    else:
        Xh = space.rvs_transformed(n_samples=n_points, random_state=rng)
        t1 = time.perf_counter()
        X = torch.from_numpy(Xh).to(dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
    top = _device_topk(est, X, y_opt, ACQS, 0.01, 1.96, 5)       # ends in the copy of the winners' indices
    t3 = time.perf_counter()
    idx = np.concatenate([top[a][1] for a in ACQS])
    starts = X[torch.from_numpy(idx).to(dev)].cpu().numpy()      # the 15 winning rows
    if frozen is None or not frozen.all():                       # an all-discrete lattice has nothing to polish
        polish_lockstep(est, list(starts), [a for a in ACQS for _ in range(5)], y_opt, 0.01, 1.96,
                        space.transformed_bounds, driver=DRIVER,
                        frozen=frozen if frozen is not None and frozen.any() else None)
    t4 = time.perf_counter()
    return dict(zip(PIECES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)))


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", default="mnist",
                    help="mnist (option3: 4 Integer + 1 Real), real10, real10int2 (ten Reals, Integer(0, 9) and "
                         "Integer(0, 19)), or several: mnist,real10")
    ap.add_argument("--n-points", type=int, default=1_000_000, dest="n_points")
    ap.add_argument("--told", type=int, default=200)
    ap.add_argument("--source", default="both", choices=["both", "all", "host", "device", "lattice"],
                    help="both: host and device; all: host, device and lattice")
    ap.add_argument("--loss", type=int, default=0, metavar="K",
                    help="K seeded MNIST-space proposals per source: the oracle EI at the trained point")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.loss:
        return loss(a.loss, a.n_points if a.n_points != 1_000_000 else 10_000)
    for name in a.space.split(","):
        if name not in SPACES:
            ap.error(f"--space {name!r}: one of {', '.join(SPACES)}")
        probe(a, name)


SPACES = {
    "mnist": mnist_space,
    "real10": lambda: [Real(0.0, 1.0) for _ in range(10)],
    "real10int2": lambda: [Real(0.0, 1.0) for _ in range(10)] + [Integer(0, 9), Integer(0, 19)],
}


def loss(k, n_points):
    """The oracle's EI (the value skopt minimises, so lower is better) at the point each source
    trains and at the transformed point its proposal returned, for k seeds."""
    from oracle import gp_ei as O

    dev = torch.device("cuda:0")
    print(f"MNIST space, 64 told points, n_points {n_points}, acq_func EI, lbfgs: oracle -EI at the proposal's "
          "transformed point -> at the trained point (after inverse_transform)", flush=True)
    rows = {s: [] for s in ("host", "device", "lattice")}
    for seed in range(k):
        rng = np.random.RandomState(1000 + seed)
        space = Space(mnist_space())
        pts = space.rvs(64, random_state=rng)
        Xt = space.transform(pts)
        y = np.sum((Xt - rng.uniform(0.2, 0.8, Xt.shape[1])) ** 2, axis=1) + 0.05 * rng.randn(64)
        line = []
        for s in rows:
            opt = Optimizer(mnist_space(), acq_func="EI", n_initial_points=10, random_state=seed, candidates=s,
                            device=dev, acq_optimizer_kwargs={"n_points": n_points})
            opt.trace = []
            opt.tell([list(p) for p in pts], [float(v) for v in y])
            x = opt.ask()
            st = O.gp_from_theta(Xt, y, *opt.trace[-1]["theta"])
            both = np.vstack([opt.next_xs_[0], space.transform([x])[0]])
            v = O.acquisition_values(*O.posterior_skopt(st, both), float(np.min(y)), "EI")
            rows[s].append(v)
            line.append(f"{s} {v[0]:.6e} -> {v[1]:.6e}")
        print(f"  seed {seed:2d}: " + "   ".join(line), flush=True)
    trained = {s: np.array([v[1] for v in r]) for s, r in rows.items()}
    for s, r in rows.items():
        rel = np.array([(v[1] - v[0]) / abs(v[0]) for v in r])
        print(f"  {s:7s} rounding changes -EI by median {np.median(rel):+.3e} (min {rel.min():+.3e}, "
              f"max {rel.max():+.3e}) of its value; trained -EI median {np.median(trained[s]):.6e}", flush=True)
    for s in ("host", "device"):
        better = int(np.sum(trained["lattice"] < trained[s]))
        ratio = np.median(trained["lattice"] / trained[s])
        print(f"  lattice trains a point of lower -EI than {s} in {better} of {k} proposals; median EI ratio "
              f"lattice / {s} = {ratio:.4f}", flush=True)


def probe(a, space_name):
    dev = torch.device("cuda:0")
    space = Space(SPACES[space_name]())
    d = space.transformed_n_dims
    rng = np.random.RandomState(1)
    Xt = space.rvs_transformed(a.told, rng)
    y = np.sum((Xt - 0.4) ** 2, axis=1) + 0.05 * rng.randn(a.told)
    est = GPModel(Xt, y, 1.5, np.linspace(0.4, 1.3, d), 0.02, device=dev)
    est.dev
    sources = {"both": ("host", "device"), "all": ("host", "device", "lattice")}.get(a.source, (a.source,))
    ms = {s: {p: [] for p in PIECES} for s in sources}
    for it in range(a.warmup + a.reps):
        for s in sources:
            t = proposal(s, space, est, a.n_points, rng, dev)
            if it >= a.warmup:
                for p in PIECES:
                    ms[s][p].append(1e3 * t[p])
    print(f"space {space_name} (d = {d}), n_points {a.n_points}, told {a.told}, {a.reps} proposals per source "
          f"after {a.warmup} warm-up, alternating; host-clock ms: median (min .. max)", flush=True)
    for s in sources:
        print(f"  {s:6s} " + "  ".join(f"{p} {np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
                                       for p, v in ms[s].items()), flush=True)
    if "host" in sources:
        h = np.median(ms["host"]["total"])
        for s in sources[1:]:
            print(f"  total host / {s} = {h / np.median(ms[s]['total']):.1f}x", flush=True)
    # the writers alone at equal rows, HIP events, beside a fill_ of the same tensor
    L = lattice_size(space)
    rows = L * max(1, -(-a.n_points // L)) if "lattice" in sources else a.n_points
    print(f"  L = {L}; {rows} rows per writer call", flush=True)
    out = torch.empty((rows, d), dtype=torch.float64, device=dev)
    event_ms(lambda: out.fill_(0.5), a.warmup)
    event_ms(lambda: sample_transformed(space, rows, 7, dev), a.warmup)
    event_ms(lambda: lattice_transformed(space, rows, 7, dev), a.warmup)
    fill, samp, latt = [], [], []
    for _ in range(a.reps):
        fill += event_ms(lambda: out.fill_(0.5), 1)
        samp += event_ms(lambda: sample_transformed(space, rows, 7, dev), 1)
        latt += event_ms(lambda: lattice_transformed(space, rows, 7, dev), 1)
    gb = out.numel() * 8 / 1e9
    for name, v in (("mpo_space_sample", samp), ("mpo_space_lattice", latt), ("fill_", fill)):
        print(f"  {name}: {np.median(v):.4f} ms ({min(v):.4f} .. {max(v):.4f}) device events, "
              f"{gb / (np.median(v) * 1e-3):.0f} GB/s written ({gb * 1e3:.1f} MB)", flush=True)


if __name__ == "__main__":
    main()
