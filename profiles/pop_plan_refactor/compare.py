"""Parent-versus-branch checks of the MNIST population plan refactor (WorkList, tallied
step work).  Run one mode once per commit and diff the two outputs: they are identical.

    python compare.py work   [--root TREE]    no GPU: mpo_pop_step_work and mpo_pop_sizes over
                                              populations x masks x MPO_POP_PLAN knobs
    python compare.py tables [--root TREE]    GPU: SHA-256 of the device tables after bind and
                                              after every set_active
    python compare.py bits   [--root TREE]    GPU: digests of a short training run with a
                                              retirement, at the defaults and with streams=1

TREE holds the ``mpi_opt_amd`` package (with its built libmpo.so) of the commit under
test; the populations come from ``tests/`` of the working directory.
"""
import argparse
import ctypes
import hashlib
import os
import sys

KNOBS = ["", "streams=1", "streams=2", "wgs=1", "dgs=2", "occmerge=0", "occmerge=1", "xcd=0", "conv_mt=2", "wgrpb=1",
         "dgfwd=0", "dgfwd=10", "wg_spg2_big=0", "PROFILE"]


def populations():
    import pop_cases
    import test_retire_host as T

    out = [("MEMBERS", T.BATCH, [pop_cases.M(*m) for m in T.MEMBERS])]
    out += [(name, pop_cases.POP[name][0], pop_cases.POP[name][1]) for name in ("b1", "b2")]   # k = 10, F = 64
    return out


def masks(members):
    n = len(members)
    nt1 = [i for i, m in enumerate(members) if (m.F + 15) // 16 == 1]
    small_k = [i for i, m in enumerate(members) if m.k <= 4]
    named = [("none", []), ("[2]", [2]), ("NT1", nt1), ("SMALL_K", small_k), ("[0,2,5]", [0, 2, 5]),
             ("all-but-one", list(range(1, n)))]
    return [(name, [i for i in r if i < n]) for name, r in named]


def set_knob(knob):
    os.environ.pop("MPO_POP_PLAN", None)
    os.environ.pop("MPO_POP_PROFILE", None)
    if knob == "PROFILE":
        os.environ["MPO_POP_PROFILE"] = "1"
    elif knob:
        os.environ["MPO_POP_PLAN"] = knob


def mask_bytes(n, retired):
    return (ctypes.c_uint8 * n)(*[0 if i in retired else 1 for i in range(n)])


def mode_work():
    from mpi_opt_amd import _lib

    L = _lib.lib()
    for pname, B, members in populations():
        for knob in KNOBS:
            set_knob(knob)
            arr = (_lib.MpoCnnSpec * len(members))()
            for i, m in enumerate(members):
                arr[i] = _lib.MpoCnnSpec(m.F, m.k, m.p, m.dense, m.lr, m.dropout, 7 + i,
                                         _lib.LOSS_CODES[m.loss] | _lib.OPT_CODES[m.optimizer])
            h = ctypes.c_void_p()
            _lib.check(L.mpo_pop_create(arr, len(members), B, ctypes.byref(h)), "mpo_pop_create")
            for mname, retired in masks(members):
                _lib.check(L.mpo_pop_set_active(h, mask_bytes(len(members), retired), None), "mpo_pop_set_active")
                a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
                _lib.check(L.mpo_pop_step_work(h, ctypes.byref(a), ctypes.byref(b)), "mpo_pop_step_work")
                sz = _lib.MpoPopSizes()
                _lib.check(L.mpo_pop_sizes(h, ctypes.byref(sz)), "mpo_pop_sizes")
                print(f"{pname} knob={knob or '-'} mask={mname} work=({a.value}, {b.value}) sizes=({sz.n_params}, "
                      f"{sz.act_floats}, {sz.table_bytes}, {sz.n_members}, {sz.batch})")
            L.mpo_pop_destroy(h)
    set_knob("")


def engine(members, B):
    from mpi_opt_amd.population import PopulationEngine, TrialSpec

    specs = [TrialSpec(m.F, m.k, m.p, m.dense, m.lr, m.dropout, 7 + i, m.loss, m.optimizer)
             for i, m in enumerate(members)]
    return PopulationEngine(specs, batch=B, device="cuda:0", init_seed=3)


def digest(t):
    import torch

    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def mode_tables():
    import numpy as np

    for pname, B, members in populations():
        eng = engine(members, B)
        print(f"{pname} bind {digest(eng.tables)}")
        for mname, retired in masks(members):
            eng.set_active(np.array([i not in retired for i in range(len(members))]))
            print(f"{pname} mask={mname} {digest(eng.tables)}")


def mode_bits():
    import numpy as np
    import torch

    pname, B, members = populations()[0]
    n = len(members)
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.rand(6 * B, 784).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, 10, 6 * B).astype(np.int32)).cuda()
    order = torch.stack([torch.from_numpy(rng.permutation(6 * B).astype(np.int32)) for _ in range(n)]).cuda()
    for knob in ("", "streams=1"):
        set_knob(knob)
        eng = engine(members, B)
        losses = []
        for step in range(4):
            if step == 2:
                eng.set_active(np.array([i not in (0, 2, 5) for i in range(n)]))
            losses.append(eng.train_step(x, y, order, step * B).clone())
        eng.eval_reset()
        eng.eval_step(x, y, order, 5 * B)
        print(f"{pname} knob={knob or '-'} params={digest(eng.params)} loss_out={digest(torch.stack(losses))} "
              f"val_loss_sum={digest(eng.val_loss_sum)} correct={digest(eng.val_correct)}")
    set_knob("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["work", "tables", "bits"])
    ap.add_argument("--root", default=os.getcwd())
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    sys.path.insert(0, os.path.abspath(args.root))
    {"work": mode_work, "tables": mode_tables, "bits": mode_bits}[args.mode]()
