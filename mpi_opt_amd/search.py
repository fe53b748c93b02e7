"""Hyper-parameter search driver: the option3 CLI on the MI355X engine.

    python -m mpi_opt_amd.search --block-size 5 --example mnist --epochs 10 \\
        --num-iterations 10 [--n-fold 5] [--world-size 21]
    python -m torch.distributed.run --nproc-per-node 8 -m mpi_opt_amd.search ...

Same flags and defaults as /root/reference/hyperparameter_search_option3.py:54-96
(make_parser) with the same sanity check (:51-52) and block arithmetic
(:174-181: ``num_blocks, left_over = divmod(size - 1, block_size)``, exit on a
leftover).  ``--world-size`` plays the role of ``mpirun -n`` (the number of
ranks the reference would have): it fixes how many trials run concurrently
(``num_blocks``).  Every trial trains as population members on the GPU(s)
instead of on MPI blocks.

Training flags: ``--loss`` (binary_crossentropy | categorical_crossentropy) and
``--optimizer`` (adam | sgd) select the member's loss and update rule in the
kernels; ``--early-stopping`` / ``--target-metric`` stop members per fold
(mpi_opt_amd.stopping); another value is refused with exit status 2.  Flags
that configure mpi_learn's Downpour/EASGD exchange (--sync-every, --easgd,
--elastic-*, --n-master, --n-process, --worker-optimizer) are accepted and
recorded but have no effect: a trial is trained synchronously on one GPU
(single-trial semantics).  ``--preload-data`` / ``--cache-data``
concern mpi_learn's file loader; the data here is resident in HBM.

``--lie-refit never`` (an addition, default ``every``) departs from the reference:
skopt refits the GP hyper-parameters for every constant-liar lie of an ask batch;
``never`` keeps the theta of the last told model for the whole batch and appends
each lie to the posterior (``mpo_gp_append``).

``--candidate-source device`` (an addition, default ``host``) departs from the
reference too: the ``--ei-candidates`` acquisition candidates of a proposal are
written on the GPU from one seed (``mpo_space_sample``, mpi_opt_amd.candidates)
instead of being drawn from the optimizer's RandomState on the host.
``--candidate-source lattice`` departs further, and is NOT the reference's semantics:
the candidates are every combination of the space's Integer and Categorical values
(``mpo_space_lattice``) and the polish moves the Real dimensions only, so the point
that is trained is a point that was scored.
"""
from __future__ import annotations

import argparse
import os
import sys


def make_parser():
    p = argparse.ArgumentParser(description="Bayesian hyper-parameter search on MI355X")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--batch", help="batch size", default=100, type=int)
    p.add_argument("--epochs", help="number of training epochs", default=10, type=int)
    p.add_argument("--optimizer", help="optimizer for master to use (adam | sgd)", default="adam")
    p.add_argument("--loss", help="loss function (binary_crossentropy | categorical_crossentropy)",
                   default="binary_crossentropy")
    p.add_argument("--sync-every", default=1, type=int, dest="sync_every",
                   help="how often to sync weights with master (no effect: synchronous single-GPU trials)")
    p.add_argument("--preload-data", default=0, type=int, dest="data_preload",
                   help="mpi_learn data preloading (no effect here: the data is resident on the GPU)")
    p.add_argument("--cache-data", default="", dest="caching_dir",
                   help="mpi_learn data cache dir (no effect here: the data is resident on the GPU)")
    p.add_argument("--early-stopping", default=None, dest="early_stopping",
                   help="patience for early stopping: N (val_loss) or METRIC,~<,N / METRIC,~>,N "
                        "(Keras EarlyStopping semantics restated from the flag's help; mpi_learn is "
                        "un-vendored, so parity unpinned)")
    p.add_argument("--target-metric", default=None, dest="target_metric",
                   help="stop a fold once METRIC,OP,VALUE holds (e.g. val_acc,>,0.97; restated from the "
                        "flag's help, parity unpinned)")
    p.add_argument("--easgd", action="store_true", help="mpi_learn EASGD exchange (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--worker-optimizer", dest="worker_optimizer", default="sgd",
                   help="mpi_learn worker optimizer (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--elastic-force", type=float, default=0.9, help="EASGD (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--elastic-lr", type=float, default=1.0, dest="elastic_lr", help="EASGD (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--elastic-momentum", type=float, default=0, dest="elastic_momentum", help="EASGD (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--block-size", type=int, default=2, help="number of ranks per block (reference MPI layout)")
    p.add_argument("--n-fold", type=int, default=1, dest="n_fold")
    p.add_argument("--n-master", type=int, default=1, dest="n_master", help="mpi_learn masters per block (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--n-process", type=int, default=1, dest="n_process",
                   help="mpi_learn processes per worker (no effect here: trials train synchronously on one GPU)")
    p.add_argument("--num-iterations", type=int, default=10)
    p.add_argument("--previous-result", default=None, dest="previous_state")
    p.add_argument("--target-objective", type=float, default=None, dest="target_objective")
    p.add_argument("--example", default="mnist", choices=["topclass", "mnist", "gan"])
    # MI355X build additions
    p.add_argument("--world-size", type=int, default=21,
                   help="rank count of the reference's `mpirun -n` (sets concurrent trials)")
    p.add_argument("--n-samples", type=int, default=60000,
                   help="synthetic samples: MNIST-shape (--example mnist) or 150x94x5 LCD-jet-shape images "
                        "(--example topclass: 282 KB per sample on the device)")
    p.add_argument("--synthetic-labels", default="uniform", choices=["uniform", "learnable"],
                   dest="synthetic_labels",
                   help="labels of the synthetic data: uniform random (SURVEY §8d; a flat objective) or a "
                        "fixed random linear teacher on the pooled image (learnable; trials differ)")
    p.add_argument("--data-dir", default=None,
                   help="directory of *.h5 files: `features` / `labels` for --example mnist (option3's "
                        "/bigdata/shared/mnist/*.h5), `Images` / `Labels` for --example topclass (option3's "
                        "LCDJets_Remake files); first 70%% of the files train, the rest validate")
    p.add_argument("--lr", type=float, default=1e-3, help="Adam learning rate (mpi_learn default)")
    p.add_argument("--history-dir", default=None, help="write per-trial history JSON here")
    p.add_argument("--checkpoint", default="coordinator.pkl")
    p.add_argument("--ei-candidates", type=int, default=10000,
                   help="acquisition candidates per ask (skopt n_points); split over the GPUs when distributed, "
                        "except with --candidate-source device, whose candidates are scored on the asking "
                        "rank's GPU and never split")
    p.add_argument("--candidate-source", default="host", choices=["host", "device", "lattice"],
                   dest="candidate_source",
                   help="where the acquisition candidates of an ask are drawn: host (skopt's RandomState "
                        "stream, copied to the GPU), device (NOT the reference's stream: one seed per "
                        "proposal, the candidates written on the GPU as a function of (seed, row); for "
                        "large --ei-candidates; scored on the asking rank's GPU) or lattice (NOT the "
                        "reference's semantics: every combination of the Integer and Categorical values is a "
                        "candidate, whole copies of that set up to --ei-candidates rows with Reals drawn as "
                        "device draws them, and the polish moves the Reals only; refused past 2^22 "
                        "combinations; scored on the asking rank's GPU)")
    p.add_argument("--chain-workers", type=int, default=8,
                   help="concurrent cl_min ask batches per GPU (worker threads, one HIP stream each; their "
                        "refit rounds share launches); 0 runs every ask inline, as the reference's "
                        "Coordinator does")
    p.add_argument("--population-chunks", type=int, default=1, dest="population_chunks",
                   help="train each population in this many parts, each as soon as its ask batches "
                        "resolve (overlaps the remaining batches with training; results unchanged)")
    p.add_argument("--lie-refit", default="every", choices=["every", "never"], dest="lie_refit",
                   help="hyper-parameter refits inside an ask batch: every (a refit per constant-liar lie, "
                        "skopt's and the reference's semantics) or never (NOT the reference's semantics: the "
                        "batch keeps the theta of the last told model and appends each lie to its posterior "
                        "in O(n^2); tells always refit)")
    p.add_argument("--batch-strategy", default="cl_min", choices=["cl_min", "thompson"], dest="batch_strategy",
                   help="how an ask batch is made: cl_min (the constant-liar batch, skopt's and the reference's "
                        "semantics) or thompson (NOT the reference's semantics: one fit per batch, one joint "
                        "draw of the posterior over n_ts_points candidates per point, each point the argmin of "
                        "its draw; no lies, no refits, no polish)")
    p.add_argument("--thompson-sampler", default="joint", choices=["joint", "paths"], dest="thompson_sampler",
                   help="how a thompson batch draws its samples: joint (the exact joint posterior over "
                        "n_ts_points <= 4096 candidates) or paths (pathwise conditioning over all "
                        "--ei-candidates: the conditioning on the data is exact, the Matern prior is a "
                        "random-Fourier-feature APPROXIMATION; nothing is known about its effect on search quality)")
    p.add_argument("--thompson-polish", action="store_true", dest="thompson_polish",
                   help="with --batch-strategy thompson --thompson-sampler paths: minimise each sample path "
                        "from its picked candidate by L-BFGS-B (20 iterations) instead of stopping at the "
                        "candidate (NOT the reference's semantics; nothing is known about its effect on "
                        "search quality)")
    p.add_argument("--surrogate", default="exact", choices=["exact", "committee"],
                   help="the optimizer's surrogate: exact (one GP over all told points, skopt's and the reference's "
                        "semantics; at most 2048 observations) or committee (NOT the reference's semantics: past "
                        "--expert-size observations the points are split over ceil(n / expert-size) exact GPs that "
                        "share one theta, combined as a robust Bayesian committee machine; up to 32 experts; "
                        "nothing is known about its effect on search quality)")
    p.add_argument("--expert-size", type=int, default=512, dest="expert_size", metavar="N",
                   help="with --surrogate committee: the most observations of one expert (16 .. 2048)")
    p.add_argument("--acq-func", default="gp_hedge", choices=list(ACQ_FUNCS), dest="acq_func",
                   help="the optimizer's acquisition function (skopt's names; the reference's Coordinator uses the "
                        "default, gp_hedge).  EIps / PIps are skopt's cost-aware acquisitions: every result is told "
                        "with a cost, and the acquisition is divided by the expected cost.  The cost here is the "
                        "MODELLED training GFLOP per sample of the trial's architecture, not a measured time, and "
                        "it ignores early stopping")
    p.add_argument("--report", default=None, metavar="PATH",
                   help="an addition of this build (NOT in the reference, which ends by printing the best "
                        "observed point): after the last tell, rank 0 writes the objective report to PATH as JSON "
                        "-- the partial dependence of every dimension and pair, each dimension's importance and "
                        "the surrogate's expected minimum (mpi_opt_amd.analysis.objective_report; its samples come "
                        "from its own seed, never from the optimizer's stream)")
    return p


#: --acq-func: skopt's acquisition functions
ACQ_FUNCS = ("gp_hedge", "EI", "PI", "LCB", "EIps", "PIps")


def modelled_cost_fn(provider):
    """cost_fn of a cost-aware search: params -> the modelled training GFLOP per sample of the
    trial (``models.flops_of_params``).  A model of the architecture, not a measurement; early
    stopping does not enter it."""
    from .models import flops_of_params

    names = [p.name for p in provider.parameters]
    return lambda params: flops_of_params(provider.model_fn, names, params) * 1e-9


#: --example -> (features_name, labels_name) of its *.h5 files (option3:122-123, 141-142)
EXAMPLE_DATASETS = {"mnist": ("features", "labels"), "topclass": ("Images", "Labels")}


def example_provider(example, input_shape=None):
    """option3:108-133: the model provider of ``--example``.  ``input_shape`` (topclass
    only): build test_cnn on images of that shape instead of the reference's 150x94x5."""
    from .models import BuilderFromFunction, mnist_space, test_cnn, test_mnist, topclass_space

    if example == "topclass":
        import functools

        fn = test_cnn if input_shape is None else functools.partial(test_cnn, input_shape=tuple(input_shape))
        return BuilderFromFunction(model_fn=fn, parameters=topclass_space())
    if example == "mnist":
        return BuilderFromFunction(model_fn=test_mnist, parameters=mnist_space())
    raise ValueError(f"example {example!r} has no population engine")


def check_sanity(args):
    assert args.block_size > 1, "Block size must be at least 2 (master + worker)"


def check_training_flags(args):
    """--loss / --optimizer / --early-stopping / --target-metric configure the
    trials' training (option3:60-61, 66-69 -> Algo and MPIKFoldManager); a value
    the population kernels do not implement is refused, never ignored.
    Returns the parsed stopping rule (or None)."""
    from . import _lib
    from .stopping import StopRule

    if args.loss not in _lib.LOSS_CODES:
        raise ValueError(f"--loss {args.loss!r}: the population kernels implement {sorted(_lib.LOSS_CODES)}")
    if args.optimizer not in _lib.OPT_CODES:
        raise ValueError(f"--optimizer {args.optimizer!r}: the population kernels implement {sorted(_lib.OPT_CODES)}")
    return StopRule.from_args(args.early_stopping, args.target_metric)


#: flags of mpi_learn's asynchronous multi-process training that have no counterpart
#: here (a trial trains synchronously on one GPU): (dest, default)
NO_EFFECT_FLAGS = (("sync_every", 1), ("data_preload", 0), ("caching_dir", ""), ("easgd", False),
                   ("worker_optimizer", "sgd"), ("elastic_force", 0.9), ("elastic_lr", 1.0),
                   ("elastic_momentum", 0), ("n_master", 1), ("n_process", 1))


def no_effect_notes(args):
    """One note per no-effect flag set away from its default (printed, not silent)."""
    return [f"note: --{dest.replace('_', '-')}={getattr(args, dest)!r} has no effect here "
            f"(mpi_learn's multi-process exchange is not reproduced; trials train synchronously on one GPU)"
            for dest, dflt in NO_EFFECT_FLAGS if getattr(args, dest, dflt) != dflt]


def block_layout(world_size, block_size):
    """option3:174-181: (num_blocks, left_over)."""
    return divmod(world_size - 1, block_size)


def run_search(args, x=None, y=None, log=print, progress=None, on_population=None):
    """Run the option3 search for parsed ``args``; returns a report dict (rank 0)
    or None (ranks > 0, which serve their shards until rank 0 is done).

    The report splits the wall time into the optimizer (ask = GP refits of the
    cl_min batch + acquisition, tell = the refit on told results) and the
    device training of the populations, and counts the trials trained."""
    import time

    import torch

    from .blocks import DistributedEvaluator, PopulationComm, ShardedScorer, TrialEvaluator
    from .chains import DistributedChainExecutor, ThreadChainExecutor
    from .population import synthetic_mnist
    from .scheduler import AskTellScheduler

    num_blocks, left_over = block_layout(args.world_size, args.block_size)
    stopping = check_training_flags(args)
    for note in no_effect_notes(args):
        log(note)
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    import torch.distributed as _dist

    # a group the caller set up is used even at world size 1 (the RCCL path under test)
    if ws > 1 or (_dist.is_available() and _dist.is_initialized()):
        dist = _dist
        if not dist.is_initialized():
            torch.cuda.set_device(local)
            dist.init_process_group("nccl")
        # a caller that set up the group (bench.py) also chose this rank's device
        local = torch.cuda.current_device()
    dev = torch.device("cuda", local)
    example = getattr(args, "example", "mnist")
    # caller-supplied topclass images set test_cnn's input shape (the reference fixes 150x94x5)
    provider = example_provider(example, tuple(x.shape[1:]) if example == "topclass" and x is not None else None)
    holdout = None
    if x is None and args.data_dir:
        from .h5 import load_xy, split_files

        import numpy as np

        train_list, val_list = split_files(args.data_dir)
        if example == "topclass":
            fn, ln = EXAMPLE_DATASETS[example]
            (xt, yt), (xv, yv) = (load_xy(lst, features_name=fn, labels_name=ln) for lst in (train_list, val_list))
            # load_xy flattens rows (NHWC order) and arg-maxes one-hot labels; test_cnn's input is 150x94x5
            if xt.shape[1] != 150 * 94 * 5 or xv.shape[1] != 150 * 94 * 5:
                raise ValueError(f"--example topclass: `Images` rows of {xt.shape[1]} values, not 150*94*5")
            xt, xv = xt.reshape(-1, 150, 94, 5), xv.reshape(-1, 150, 94, 5)
        else:
            (xt, yt), (xv, yv) = load_xy(train_list), load_xy(val_list)
        holdout = len(yt)
        xh, yh = np.concatenate([xt, xv]), np.concatenate([yt, yv])
        x, y = torch.from_numpy(xh).to(dev), torch.from_numpy(yh).to(dev)
        log(f"data: {len(train_list)} train / {len(val_list)} validation files, {holdout} / "
            f"{len(yh) - holdout} samples")
    if x is None and example == "topclass":
        from .topclass import synthetic_topclass

        x, y = synthetic_topclass(args.n_samples, seed=0, device=dev, labels=args.synthetic_labels)
    if x is None:
        x, y = synthetic_mnist(args.n_samples, seed=0, device=dev, labels=args.synthetic_labels)
    evaluator = TrialEvaluator(provider, x, y, n_fold=args.n_fold, epochs=args.epochs, batch=args.batch,
                               lr=args.lr, device=dev, history_dir=args.history_dir, holdout=holdout,
                               progress=progress if (dist is None or dist.get_rank() == 0) else None,
                               loss=args.loss, optimizer=args.optimizer, stopping=stopping)
    local_eval = evaluator
    chains = None
    if args.chain_workers > 0:
        chains = ThreadChainExecutor(dev, workers=args.chain_workers)
    if dist is not None:
        evaluator = DistributedEvaluator(evaluator)
        if chains is not None:
            chains = DistributedChainExecutor(evaluator, chains)
        if evaluator.rank != 0:
            try:
                evaluator.serve()
            finally:
                if chains is not None:
                    chains.close()
            return None
    comm = PopulationComm(num_blocks, args.block_size, evaluator, chunks=args.population_chunks)

    def _population_done(i, entry):
        from . import optimizer as _o

        log(f"population {i}: {entry[3]} trials; {entry[0]:.1f} s before it, {entry[1]:.1f} s waiting for ask "
            f"batches, {entry[2]:.1f} s training; {_o.STATS['refits']} refits so far")
        if on_population is not None:
            on_population(i, entry, dict(_o.STATS))

    comm.on_population = _population_done
    opt_kw = {"device": dev, "acq_optimizer_kwargs": {"n_points": args.ei_candidates}}
    if args.lie_refit != "every":
        opt_kw["lie_refit"] = args.lie_refit              # fixed-theta ask batches (not skopt's semantics)
    if args.batch_strategy != "cl_min":
        opt_kw["batch_strategy"] = args.batch_strategy    # Thompson ask batches (not skopt's semantics)
    if args.surrogate != "exact":
        opt_kw["surrogate"] = args.surrogate              # a committee of experts (not skopt's semantics)
    if args.expert_size != 512:
        opt_kw["expert_size"] = args.expert_size
    if args.candidate_source != "host":
        opt_kw["candidates"] = args.candidate_source      # written on the device (not skopt's stream)
    if args.thompson_sampler != "joint":
        # pathwise Thompson draws over all --ei-candidates (a random-feature prior; not skopt's semantics)
        opt_kw["acq_optimizer_kwargs"]["ts_sampler"] = args.thompson_sampler
    if getattr(args, "thompson_polish", False):
        opt_kw["acq_optimizer_kwargs"]["ts_polish"] = True    # each draw minimised from its pick
    cost_fn = None
    if args.acq_func != "gp_hedge":
        opt_kw["acq_func"] = args.acq_func
    if args.acq_func.endswith("ps"):
        cost_fn = modelled_cost_fn(provider)              # told as (fom, cost) pairs
    if chains is not None:
        opt_kw["chain_executor"] = chains                 # ask batches run concurrently (mpi_opt_amd.chains)
    if dist is not None:
        opt_kw["scorer"] = ShardedScorer(evaluator)       # candidates split M/W over the GPUs
    sched = AskTellScheduler(comm, num_blocks, provider.parameters, checkpoint=args.checkpoint,
                             target_fom=args.target_objective, verbose=args.verbose, optimizer_kwargs=opt_kw,
                             cost_fn=cost_fn)
    from . import optimizer as _opt_mod

    _opt_mod.reset_stats()
    if args.previous_state:
        sched.load(args.previous_state)
        # the pickle carries no device state: re-attach this run's device and scorer
        sched.optimizer.set_runtime(device=dev, scorer=opt_kw.get("scorer"), chain_executor=chains)
    t0 = time.perf_counter()
    try:
        state = sched.run(num_iterations=args.num_iterations)
        wall = time.perf_counter() - t0
    except BaseException:
        if chains is not None:      # do not run the queued batches before the error surfaces
            (getattr(chains, "local", None) or chains).cancel("search failed")
        raise
    finally:
        if dist is not None:
            evaluator.shutdown()
        if chains is not None:
            chains.close()
    tm = sched.timings
    chain_wait = chains.wait_s if chains is not None else 0.0
    report = {
        "wall_s": wall,
        "trials_trained": comm.trials_trained,
        "trials_told": len(state.fom_list),
        "populations": list(comm.batches),
        "trained_params": [list(p) for p in comm.trained_params],
        "told_params": [list(p) for p in state.param_list], "told_foms": list(state.fom_list),
        "num_blocks": num_blocks,
        # seconds the search loop spent on the optimizer: asks (inline batches, or just
        # recording a lazy one), tells, and waiting for lazy batches before a population trains
        "optimizer_s": tm["ask_s"] + tm["tell_s"] + chain_wait,
        "ask_s": tm["ask_s"], "tell_s": tm["tell_s"], "asks": tm["asks"], "tells": tm["tells"],
        "chain_wait_s": chain_wait, "chain_workers": args.chain_workers,
        "population_chunks": args.population_chunks,
        "chain_pool": f"{args.chain_workers} threads" if chains is not None else None,
        "chain_busy_s": chains.busy_s if chains is not None else 0.0,
        # seconds each ask batch ran on its worker, in submission order (one per ask)
        "chain_run_s": [d for _, d in sorted(getattr(chains, "durations", []) or
                                             getattr(getattr(chains, "local", None), "durations", []))],
        "train_s": local_eval.train_s,
        # headline on TOLD trials (the ones the optimizer saw); the in-flight tail the
        # exit barrier trains (coordinator.py:98-101 never tells it) is reported apart
        "trials_per_hour": 3600.0 * len(state.fom_list) / wall if wall > 0 else None,
        "trained_per_hour": 3600.0 * comm.trials_trained / wall if wall > 0 else None,
        "tail_trials": len(comm.tail),
        # per population: [between populations (tells, asks, launches), waiting for ask batches, training, trials]
        "timeline": [list(t) for t in comm.timeline],
        "best_fom": state.best_fom, "best_params": state.best_params,
        "gp": dict(_opt_mod.STATS),     # refits (tell + every cl_min lie), their n, refit / proposal seconds
    }
    if getattr(args, "report", None):
        from .analysis import objective_report, write_report

        write_report(objective_report(sched.optimizer), args.report)
        report["report"] = args.report
        log(f"objective report written to {args.report}")
    log(f"search done: {report['trials_trained']} trials trained ({report['trials_told']} told) in "
        f"{wall:.1f} s; optimizer {report['optimizer_s']:.2f} s, training {report['train_s']:.1f} s; "
        f"best {state.best_fom} at {state.best_params}")
    return report


def main(argv=None):
    args = make_parser().parse_args(argv)
    check_sanity(args)
    try:
        check_training_flags(args)
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    if args.thompson_polish and (args.batch_strategy != "thompson" or args.thompson_sampler != "paths"):
        print("error: --thompson-polish needs --batch-strategy thompson --thompson-sampler paths "
              "(only a sample path is a function that can be minimised)", file=sys.stderr)
        return 2
    if args.example not in EXAMPLE_DATASETS:
        print(f"example {args.example!r}: its data (3D GAN) and model are outside the population engines, "
              f"which train the examples {sorted(EXAMPLE_DATASETS)}", file=sys.stderr)
        return 2
    num_blocks, left_over = block_layout(args.world_size, args.block_size)
    if left_over:
        print("The last block is going to be made of {} nodes, make inconsistent block size {}".format(
            left_over, args.block_size))
        return 1
    run_search(args)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
