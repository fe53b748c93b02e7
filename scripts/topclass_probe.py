"""Measure one train step of a topclass population (csrc/topclass.hip) on the GPU.

    python scripts/topclass_probe.py [--members 64 --batch 100 --steps 5 --warmup 2] [--out FILE]

Workload: ``members`` test_cnn members x ``batch`` samples at 150x94x5, kernel_size and
dropout drawn from option3's topclass space (seeded), member i on fold i % 5 of a 5-fold
split, as a search would run them.  Prints one JSON line: device ms per step (HIP events),
the modelled FLOP (``TopclassSpec.flops_per_sample_train``) and its fraction of the
157.3 TFLOP/s fp32 MFMA rate, and two models of the bytes of x a step must read: once per
member and pass (what the engine does: conv1 forward and conv1 weight gradient each gather
x per member) and once per sharing group (members with the same kernel_size and order row
could share one staged im2col tile).

Counters need runs of their own (one counter per run):

    rocprofv3 --pmc FETCH_SIZE -d DIR_F -o pmc --output-format csv -- \\
        python scripts/topclass_probe.py --steps 1 --warmup 0
    rocprofv3 --pmc WRITE_SIZE -d DIR_W ...   (the same)
    python scripts/topclass_probe.py --fold-pmc DIR_F DIR_W [--out FILE]

``--fold-pmc`` needs no GPU: it sums the counters over the tc_* kernels of the one step.
FETCH_SIZE / WRITE_SIZE are KiB at the L2's memory side; they are reported as counted (the
doubling that applies to 16 B/lane streaming reads is not calibrated for this engine's
4 B/lane gathers).
"""
import argparse
import collections
import csv
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
SHAPE, CLASSES, N_FOLD = (150, 94, 5), 3, 5


def population(members, batch):
    import numpy as np

    from mpi_opt_amd.models import topclass_space
    from mpi_opt_amd.space import Space
    from mpi_opt_amd.topclass import TopclassSpec

    pts = Space(topclass_space()).rvs(n_samples=members, random_state=np.random.RandomState(0))
    return [TopclassSpec(kernel_size=int(p[1]), dropout=float(p[0]), seed=i, input_shape=SHAPE, classes=CLASSES)
            for i, p in enumerate(pts)]


def x_models(specs, batch):
    per_pass = batch * SHAPE[0] * SHAPE[1] * SHAPE[2] * 4
    groups = len({(s.kernel_size, i % N_FOLD) for i, s in enumerate(specs)})
    return {"x_bytes_per_sample_pass": per_pass // batch, "sharing_groups": groups,
            "x_once_per_member_bytes": 2 * len(specs) * per_pass, "x_once_per_group_bytes": 2 * groups * per_pass}


def measure(args):
    import numpy as np
    import torch

    from mpi_opt_amd.population import kfold_split
    from mpi_opt_amd.topclass import TopclassPopulation, synthetic_topclass

    specs = population(args.members, args.batch)
    n = max(args.n_samples, 2 * N_FOLD * args.batch)
    x, y = synthetic_topclass(n, SHAPE, CLASSES, seed=0, device="cuda:0")
    order = torch.from_numpy(np.stack([kfold_split(n, N_FOLD, i % N_FOLD)[0][:n - n // N_FOLD - 1]
                                       for i in range(len(specs))])).cuda()
    pop = TopclassPopulation(specs, batch=args.batch, device="cuda:0")
    for _ in range(args.warmup):
        pop.train_step(x, y, order, 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    ev[0].record()
    for i in range(args.steps):
        pop.train_step(x, y, order, 0)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
    flop = sum(s.flops_per_sample_train() for s in specs) * args.batch
    best = min(ms)
    out = {"members": len(specs), "batch": args.batch, "shape": list(SHAPE),
           "kernel_sizes": dict(sorted(collections.Counter(s.kernel_size for s in specs).items())),
           "ms_per_step": ms, "ms_per_step_min": best, "ms_per_step_median": float(np.median(ms)),
           "model_gflop_per_step": flop * 1e-9, "tflops": flop / (best * 1e-3) * 1e-12,
           "fraction_of_f32_mfma_peak": flop / (best * 1e-3) / PEAK_F32_MFMA,
           "loss_finite": bool(torch.isfinite(pop.loss).all().item())}
    out.update(x_models(specs, args.batch))
    out["x_once_per_member_gbs_at_min"] = out["x_once_per_member_bytes"] / (best * 1e-3) * 1e-9
    return out


def fold_pmc(dirs, args):
    tot, by = collections.Counter(), collections.defaultdict(collections.Counter)
    for d in dirs:
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                name = r["Kernel_Name"]
                if "tc_" not in name:
                    continue
                fam = re.search(r"tc_\w+(?:<[^>]*>)?", name).group(0)
                tot[r["Counter_Name"]] += float(r["Counter_Value"])
                by[fam][r["Counter_Name"]] += float(r["Counter_Value"])
    out = {"fetch_bytes": tot.get("FETCH_SIZE", 0.0) * 1024, "write_bytes": tot.get("WRITE_SIZE", 0.0) * 1024,
           "by_kernel_KiB": {k: dict(v) for k, v in sorted(by.items())}}
    out.update(x_models(population(args.members, args.batch), args.batch))
    out["fetch_over_x_once_per_member"] = out["fetch_bytes"] / out["x_once_per_member_bytes"]
    out["fetch_over_x_once_per_group"] = out["fetch_bytes"] / out["x_once_per_group_bytes"]
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--members", type=int, default=64)
    p.add_argument("--batch", type=int, default=100)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--n-samples", type=int, default=1000)
    p.add_argument("--fold-pmc", nargs="+", default=None, metavar="DIR")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = fold_pmc(args.fold_pmc, args) if args.fold_pmc else measure(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
