"""What retiring half of a population saves per train step (diagnostic; bench.py has
the contract).  For the bench's 320-member MNIST population and its 32-member
DenseNet one, in one process:

  (a) a train step with every member active -- what a half-stopped population costs
      without set_active;
  (b) the same engine with the odd-indexed members retired (every trial keeps folds,
      so every bucket keeps members);
  (c) a fresh engine built from only that half -- the floor.

Each figure is the median of ``--runs`` alternating runs (a, b, c, a, b, c, ...) of
``--steps`` steps between device events; min and max give the spread.  Prints one
JSON line per engine."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd.population import PopulationEngine, TrialSpec, kfold_split, synthetic_mnist  # noqa: E402


def timed(step, steps):
    """Device ms per step over ``steps`` steps (warmed by the caller)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        step(s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(variants, runs, steps):
    """variants: {name: (prepare, step)}; prepare() runs before each timed window."""
    out = {k: [] for k in variants}
    for _ in range(runs):
        for name, (prepare, step) in variants.items():
            prepare()
            for s in range(2):
                step(s)                       # warm this variant's launches
            torch.cuda.synchronize()
            out[name].append(timed(step, steps))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
            for k, v in out.items()}


def sample_trials(n, seed):
    """bench.py's population: the option3 mnist space plus a per-trial lr and dropout."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        F, p, k, dense = (int(rng.randint(10, 51)), int(rng.randint(2, 11)), int(rng.randint(2, 11)),
                          int(rng.randint(50, 201)))
        out.append(TrialSpec(nb_filters=F, pool_size=p, kernel_size=k, dense=dense,
                             lr=float(10.0 ** rng.uniform(-4, -2)), dropout=float(rng.uniform(0.0, 0.5)), seed=i))
    return out


def mnist(args):
    B, n_fold = 100, 5
    members, folds = [], []
    for t in sample_trials(args.trials, seed=13579):
        for f in range(n_fold):
            members.append(TrialSpec(t.nb_filters, t.kernel_size, t.pool_size, t.dense, t.lr, t.dropout,
                                     seed=len(members)))
            folds.append(f)
    n = len(members)
    keep = np.arange(n) % 2 == 0
    x, y = synthetic_mnist(60000, seed=0)
    tr = np.stack([kfold_split(60000, n_fold, f)[0] for f in folds])
    order = torch.from_numpy(tr).cuda()
    order_half = torch.from_numpy(tr[keep]).cuda()
    full = PopulationEngine(members, batch=B)
    half = PopulationEngine([m for m, k in zip(members, keep) if k], batch=B)
    all_on = np.ones(n, dtype=bool)
    res = alternate({
        "a_all_active": (lambda: full.set_active(all_on), lambda s: full.train_step(x, y, order, s * B)),
        "b_half_retired": (lambda: full.set_active(keep), lambda s: full.train_step(x, y, order, s * B)),
        "c_fresh_half": (lambda: None, lambda s: half.train_step(x, y, order_half, s * B)),
    }, args.runs, args.steps)
    full.set_active(keep)
    res["work_b"], res["work_c"] = full.step_work(), half.step_work()
    full.set_active(all_on)
    res["work_a"] = full.step_work()
    return {"engine": "mnist", "members": n, "steps": args.steps, "runs": args.runs, **res}


def densenet(args):
    from mpi_opt_amd.densenet import DenseNetArch, DenseNetPopulation, synthetic_cifar

    B, n = 100, args.dn_trials
    lrs = 10.0 ** np.random.RandomState(2024).uniform(-5, 1, size=n)
    keep = np.arange(n) % 2 == 0
    x, y = synthetic_cifar(50000, seed=0)
    tr, _ = kfold_split(50000, 1, 0)
    order = torch.from_numpy(np.stack([tr] * n)).cuda()
    order_half = torch.from_numpy(np.stack([tr] * int(keep.sum()))).cuda()
    full = DenseNetPopulation(DenseNetArch(), lrs, batch=B)
    half = DenseNetPopulation(DenseNetArch(), lrs[keep], batch=B)
    all_on = np.ones(n, dtype=bool)
    res = alternate({
        "a_all_active": (lambda: full.set_active(all_on), lambda s: full.train_step(x, y, order, s * B)),
        "b_half_retired": (lambda: full.set_active(keep), lambda s: full.train_step(x, y, order, s * B)),
        "c_fresh_half": (lambda: None, lambda s: half.train_step(x, y, order_half, s * B)),
    }, args.runs, args.steps)
    full.set_active(keep)
    res["work_b"], res["work_c"] = full.step_work(), half.step_work()
    full.set_active(all_on)
    res["work_a"] = full.step_work()
    return {"engine": "densenet", "members": n, "steps": args.steps, "runs": args.runs, **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=64, help="MNIST trials (x 5 folds = members)")
    ap.add_argument("--dn-trials", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--engine", choices=("mnist", "densenet", "both"), default="both")
    args = ap.parse_args()
    if args.engine in ("mnist", "both"):
        print(json.dumps(mnist(args)), flush=True)
    if args.engine in ("densenet", "both"):
        print(json.dumps(densenet(args)), flush=True)


if __name__ == "__main__":
    main()
