"""Parent-versus-branch checks of the shared population routines (csrc/pop_common.h, the
Python base class).  Run one mode once per commit and diff the two outputs.

    python compare.py asm PARENT.s BRANCH.s   no GPU: which kernels' text differs between two
                                              `hipcc ... -cuid=pin --cuda-device-only -S` files,
                                              and their VGPRs / SGPRs / scratch on both sides
    python compare.py bits [--root TREE]      GPU: digests of 3 train steps and 1 eval step of an
                                              MNIST, a topclass and a DenseNet population

TREE holds the ``mpi_opt_amd`` package (with its built libmpo.so) of the commit under
test; the populations come from ``tests/`` of the working directory.
"""
import argparse
import hashlib
import os
import re
import sys


# ---- asm ----------------------------------------------------------------------------------
def kernels(path):
    """{kernel: its text from .type to .Lfunc_end}, {kernel: (vgprs, sgprs, scratch bytes)}."""
    text, res, name, cur, meta = {}, {}, None, None, {}
    for line in open(path):
        m = re.match(r"\s+\.type\s+(\S+),@function", line)
        if m:
            name, cur = m.group(1), []
        if cur is not None:
            cur.append(line)
            if line.startswith(".Lfunc_end"):
                text[name], cur = "".join(cur), None
        m = re.match(r"    \.(name|vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\S+)", line)
        if m:
            meta[m.group(1)] = m.group(2)
            if m.group(1) == "vgpr_count":       # the last of the four keys of a kernel's entry
                res[meta["name"]] = (int(meta["vgpr_count"]), int(meta["sgpr_count"]),
                                     int(meta["private_segment_fixed_size"]))
    return text, res


def mode_asm(parent, branch):
    pt, pr = kernels(parent)
    bt, br = kernels(branch)
    assert list(pt) == list(bt), "the two files do not hold the same kernels in the same order"
    changed = [k for k in pt if pt[k] != bt[k]]
    print(f"{os.path.basename(branch)}: {len(pt)} kernels, {len(pt) - len(changed)} byte-identical, "
          f"{len(changed)} changed")
    for k in changed:
        print(f"  {k}: vgprs {pr[k][0]} -> {br[k][0]}, sgprs {pr[k][1]} -> {br[k][1]}, "
              f"scratch {pr[k][2]} -> {br[k][2]}")


# ---- bits ---------------------------------------------------------------------------------
def digest(t):
    import torch

    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def run(name, eng, x, y, B, n):
    import numpy as np
    import torch

    rng = np.random.RandomState(5)
    order = torch.stack([torch.from_numpy(rng.permutation(x.shape[0]).astype(np.int32)) for _ in range(n)]).cuda()
    losses = [eng.train_step(x, y, order, step * B).clone() for step in range(3)]
    eng.eval_reset()
    eng.eval_step(x, y, order, 3 * B)
    print(f"{name} params={digest(eng.params)} loss_out={digest(torch.stack(losses))} "
          f"val_loss_sum={digest(eng.val_loss_sum)} correct={digest(eng.val_correct)}")


def mode_bits():
    import numpy as np
    import torch

    import dn_cases
    import pop_cases
    import test_retire_host as T
    import topclass_cases
    from mpi_opt_amd.densenet import DenseNetArch, DenseNetPopulation
    from mpi_opt_amd.population import PopulationEngine, TrialSpec
    from mpi_opt_amd.topclass import TopclassPopulation, TopclassSpec

    rng = np.random.RandomState(5)
    # (a) MNIST: test_retire_host's members (BCE + Adam) and a CCE, an SGD and a CCE + SGD member
    members = [pop_cases.M(*m) for m in T.MEMBERS]
    members += [pop_cases.M(12, 3, 2, 40, loss=pop_cases.CCE), pop_cases.M(20, 4, 3, 30, optimizer="sgd"),
                pop_cases.M(8, 5, 2, 16, loss=pop_cases.CCE, optimizer="sgd")]
    B = T.BATCH
    specs = [TrialSpec(m.F, m.k, m.p, m.dense, m.lr, m.dropout, 7 + i, m.loss, m.optimizer)
             for i, m in enumerate(members)]
    x = torch.from_numpy(rng.rand(4 * B, 784).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, 10, 4 * B).astype(np.int32)).cuda()
    run("mnist", PopulationEngine(specs, batch=B, device="cuda:0", init_seed=3), x, y, B, len(specs))
    # (b) topclass: k = 1, 2, 3, 5 with BCE, CCE, SGD and Adam in one population
    c = next(c for c in topclass_cases.CASES if c.name == "mixed_k_1_2_3_5")
    specs = [TopclassSpec(kernel_size=k, dropout=d, seed=7 + i, input_shape=c.shape, classes=c.classes, loss=lo,
                          optimizer=op) for i, (k, d, lo, op) in enumerate(c.members)]
    B = c.batch
    x = torch.from_numpy(rng.rand(4 * B, *c.shape).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, c.classes, 4 * B).astype(np.int32)).cuda()
    run("topclass", TopclassPopulation(specs, batch=B, device="cuda:0", init_seed=3), x, y, B, len(specs))
    # (c) DenseNet: the 2 x 2 image of dn_cases
    c = dn_cases.BY_NAME["head1"]
    arch = DenseNetArch(img_dim=c.img, nb_classes=c.classes, depth=c.depth, nb_dense_block=c.blocks,
                        growth_rate=c.growth, nb_filter=c.nbf)
    B = c.B
    x = torch.from_numpy(rng.rand(4 * B, *c.img).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, c.classes, 4 * B).astype(np.int32)).cuda()
    eng = DenseNetPopulation(arch, [1e-3, 3e-3], batch=B, device="cuda:0", init_seed=3)
    run("densenet", eng, x, y, B, 2)
    print(f"densenet state={digest(eng.state)} penalty={digest(eng.penalty())}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["asm", "bits"])
    ap.add_argument("files", nargs="*")
    ap.add_argument("--root", default=os.getcwd())
    args = ap.parse_args()
    if args.mode == "asm":
        mode_asm(*args.files)
    else:
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        sys.path.insert(0, os.path.abspath(args.root))
        mode_bits()
