"""The lattice candidate source on the GPU: ``mpo_space_lattice`` against a numpy restatement
of its law (include/mpo.h; every comparison is ``np.array_equal``), the proposal of
``Optimizer(candidates="lattice")`` against the oracle's argmin over all legal points, the
frozen polish on a mixed space against scipy under per-run bounds, and determinism."""
import itertools

import numpy as np
import pytest
import torch
from scipy.optimize import fmin_l_bfgs_b

from mpi_opt_amd import _lib
from mpi_opt_amd.candidates import dim_table, frozen_columns, lattice_size, lattice_transformed
from mpi_opt_amd.models import mnist_space
from mpi_opt_amd.optimizer import Optimizer, acq_code
from mpi_opt_amd.space import Categorical, Integer, Real, Space
from oracle import gp_ei as O
from tests import philox_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = (0x9E3779B9 << 32) | 0x12345                 # both key words in use

#: the bar tests/test_gp_gpu.py grants acquisition values against the oracle (rtol, atol)
ACQ_RTOL, ACQ_ATOL = 1e-10, 1e-300


# ---- bits -----------------------------------------------------------------------------------

def radices(dims):
    return [dim.high - dim.low + 1 if isinstance(dim, Integer) else len(dim.categories)
            for dim in dims if isinstance(dim, (Integer, Categorical))]


def lattice_ref(dims, m, seed, first=0):
    """Rows first .. first + m - 1 of the lattice candidates of ``seed``: the Real columns of
    ``philox_ref.sample_transformed``, the discrete ones the digits of row mod L in
    ``itertools.product`` order (the last discrete dimension fastest)."""
    out = P.sample_transformed(dims, m, seed, first=first)
    rad = radices(dims)
    L = int(np.prod([int(r) for r in rad], dtype=object)) if rad else 1
    point = (np.arange(m, dtype=np.int64) + np.int64(first)) % np.int64(L)
    digits = np.unravel_index(point, rad) if rad else ()
    if L <= 4096:                                       # unravel_index IS the product order
        table = np.array(list(itertools.product(*[range(r) for r in rad])), dtype=np.int64).reshape(L, len(rad))
        assert all(np.array_equal(table[point, j], digits[j]) for j in range(len(rad)))
    col, j = 0, 0
    for dim in dims:
        w = dim.transformed_size
        if isinstance(dim, Integer):
            s = dim.high - dim.low
            out[:, col] = 0.0 if s == 0 else digits[j].astype(np.float64) / float(s)
        elif isinstance(dim, Categorical):
            out[:, col:col + w] = digits[j][:, None] if w == 1 else digits[j][:, None] == np.arange(w)
        j += isinstance(dim, (Integer, Categorical))
        col += w
    return out


def device(dims, m, first=0, seed=SEED):
    return lattice_transformed(Space(dims), m, seed, DEV, first=first).cpu().numpy()


SPACES = {
    "integers": [Integer(0, 2), Integer(5, 5), Integer(-1, 1)],                        # L = 9
    "categories": [Categorical("abc"), Integer(0, 1), Categorical("ab")],               # L = 12, a one-hot block
    # Reals in both halves of a Philox pair, and a pair that is half Real, half digit; L = 6
    "mixed": [Real(0.0, 1.0), Integer(0, 2), Real(-2.0, 2.0), Real(1e-3, 1.0, prior="log-uniform"), Integer(1, 2)],
}


@pytest.mark.parametrize("name", list(SPACES))
def test_rows_equal_the_restated_law(name):
    dims = SPACES[name]
    L = lattice_size(dims)
    d = Space(dims).transformed_n_dims
    assert (L, d) == {"integers": (9, 3), "categories": (12, 5), "mixed": (6, 5)}[name]
    # one row; one short of, exactly and one past a block; several blocks; first > 0; slices across r = L
    for first, m in ((0, 1), (0, 255), (0, 256), (0, 257), (0, 1000), (5, 333), (L - 2, 7), (3 * L - 1, 4097)):
        got = device(dims, m, first)
        assert got.shape == (m, d) and got.dtype == np.float64
        assert np.array_equal(got, lattice_ref(dims, m, SEED, first)), (name, first, m)
    whole = device(dims, 1000)
    assert np.array_equal(np.concatenate([device(dims, 77), device(dims, 923, first=77)]), whole)
    # the discrete columns repeat with period L; where there are Reals they do not
    fz = frozen_columns(dims)
    assert np.array_equal(whole[:L, fz], whole[L:2 * L, fz])
    assert len(np.unique(whole[:L, fz], axis=0)) == L
    if not fz.all():
        assert not np.array_equal(whole[:L, ~fz], whole[L:2 * L, ~fz])
        assert np.array_equal(whole[:, ~fz], P.sample_transformed(dims, 1000, SEED)[:, ~fz])
        assert not np.array_equal(whole, device(dims, 1000, seed=SEED + 1))


def test_integer_columns_are_the_transform_grid():
    dims = mnist_space()[:4]
    got = device(dims[1:3], 81)                                                         # 9 x 9: the whole lattice
    pts = list(itertools.product(range(2, 11), range(2, 11)))
    assert np.array_equal(got, Space(dims[1:3]).transform([list(p) for p in pts]))
    back = Space(dims[1:3]).inverse_transform(got)
    assert [tuple(p) for p in back] == pts


def test_whole_mnist_lattice_over_several_passes():
    """3 pairs x 200 000 rows: more (row, pair) items than the capped grid's 2^19 threads, so
    threads take a second item through the stride's carry; the slice crosses r = L = 501 471."""
    dims = mnist_space()
    L = lattice_size(dims)
    first, m = L - 120_000, 200_000
    got = device(dims, m, first)
    assert np.array_equal(got, lattice_ref(dims, m, SEED, first))
    assert (got[L - first - 1, :4] == 1.0).all() and (got[L - first, :4] == 0.0).all()  # point L - 1, then point 0


def test_lattice_past_32_bits_takes_the_64_bit_decode():
    """L = (2^31 + 1) * 6 >= 2^32: the digits come from 64-bit arithmetic, around r = L and far
    past the 32-bit rows."""
    dims = [Integer(0, 2 ** 31), Real(0.0, 1.0), Integer(0, 1), Categorical("abc")]
    L = lattice_size(dims)
    assert L == (2 ** 31 + 1) * 6 > 2 ** 32
    for first, m in ((0, 300), (L - 150, 300), (2 ** 32 - 100, 300), (5 * L + 2 ** 33 + 7, 300)):
        assert np.array_equal(device(dims, m, first), lattice_ref(dims, m, SEED, first)), first
    # just under 2^32 the 32-bit decode gives the same integers, for rows past 2^32 too
    dims = [Integer(0, 2 ** 28 - 1), Real(0.0, 1.0), Integer(0, 6), Categorical("ab")]
    L = lattice_size(dims)
    assert L == 2 ** 28 * 14 < 2 ** 32
    for first, m in ((L - 150, 300), (2 ** 32 - 100, 300)):
        assert np.array_equal(device(dims, m, first), lattice_ref(dims, m, SEED, first)), first


def test_no_rows():
    out = lattice_transformed(Space(SPACES["mixed"]), 0, SEED, DEV)
    assert tuple(out.shape) == (0, 5)
    table, d = dim_table(Space(SPACES["mixed"]))
    assert _lib.lib().mpo_space_lattice(table, len(table), d, SEED, 7, 0, None, _lib.stream_handle(DEV)) == 0


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name, m", [("integers", 65), ("categories", 64), ("mixed", 4097)])
def test_writes_stay_inside_an_output_at_either_alignment(name, m, offset):
    """The ABI on a buffer that is 16 B aligned (offset 0) or only 8 B aligned (offset 1), with
    guard words on both sides."""
    table, d = dim_table(Space(SPACES[name]))
    guard = 4
    buf = torch.full((guard + offset + m * d + guard,), -7.0, dtype=torch.float64, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lo = guard + offset
    _lib.check(_lib.lib().mpo_space_lattice(table, len(table), d, SEED, 5, m, buf.data_ptr() + 8 * lo,
                                            _lib.stream_handle(DEV)), "mpo_space_lattice")
    host = buf.cpu().numpy()
    assert np.array_equal(host[lo:lo + m * d].reshape(m, d), lattice_ref(SPACES[name], m, SEED, 5))
    assert (host[:lo] == -7.0).all() and (host[lo + m * d:] == -7.0).all()


# ---- the proposal is the lattice argmin ----------------------------------------------------------

DISCRETE = [Integer(0, 6), Integer(0, 4), Integer(0, 9)]                                # L = 350
#: chosen on the CPU with the oracle alone (its refit of these 16 points, its posterior over the
#: 350 points): the best and the runner-up differ by 5e-2 relative or more under EI, LCB and PI
ARGMIN_SEED = 6


def told_quadratic(space, seed, n=16):
    """``n`` points of ``space`` and a quadratic bowl of their transformed coordinates, its
    centre and 0.05 N(0, 1) of observation noise drawn from the same seed."""
    rng = np.random.RandomState(seed)
    pts = space.rvs(n, random_state=rng)
    centre = rng.uniform(0.2, 0.8, space.transformed_n_dims)
    y = np.sum((space.transform(pts) - centre) ** 2, axis=1) + 0.05 * rng.randn(n)
    return [list(p) for p in pts], [float(v) for v in y]


def oracle_state(opt):
    amp, ls, noise = opt.trace[-1]["theta"]
    model = opt.models[-1]
    return O.gp_from_theta(model.Xt, model.y, amp, ls, noise)


@pytest.mark.parametrize("acq, acq_optimizer", [("EI", "lbfgs"), ("LCB", "lbfgs"), ("PI", "lbfgs"),
                                                ("EI", "sampling")])
def test_proposal_is_the_lattice_argmin(acq, acq_optimizer):
    opt = Optimizer(DISCRETE, acq_func=acq, acq_optimizer=acq_optimizer, n_initial_points=8,
                    random_state=ARGMIN_SEED, candidates="lattice", device=DEV)
    opt.trace = []
    X, y = told_quadratic(opt.space, ARGMIN_SEED)
    opt.tell(X, y)
    x = opt.ask()
    rec = opt.trace[-1]
    assert rec["lattice"] == 350 and isinstance(rec["cand_seed"], int)
    assert len(rec["top"][acq]) == 1 and rec["polished"] == {}          # nothing to polish: the best candidate
    assert int(rec["top"][acq][0]) < 350                                # of 29 copies, the first

    points = [list(p) for p in itertools.product(range(7), range(5), range(10))]
    st = oracle_state(opt)
    mu, sd = O.posterior_skopt(st, opt.space.transform(points))
    v = O.acquisition_values(mu, sd, float(np.min(y)), acq)
    best = O.argmin_lowest(v)
    runner_up = np.partition(v, 1)[1]
    bar = ACQ_RTOL * abs(v[best]) + ACQ_ATOL
    got = points.index(list(x))
    print(f"{acq}/{acq_optimizer}: oracle best {points[best]} {v[best]:.6e}, runner-up {runner_up:.6e}, "
          f"gap / bar {(runner_up - v[best]) / bar:.3e}; device {x} {v[got]:.6e}")
    assert abs(v[got] - v[best]) <= bar
    assert runner_up - v[best] > 100 * bar              # the seed's choice: no near-tie, in any case
    assert got == best and int(rec["top"][acq][0]) == best


# ---- a mixed space: the polish moves the Reals only ----------------------------------------------

MIXED = [Real(0.0, 1.0), Integer(0, 5), Real(-3.0, 3.0)]


def test_mixed_space_polish_holds_the_discrete_column():
    opt = Optimizer(MIXED, acq_func="gp_hedge", n_initial_points=8, random_state=3, candidates="lattice",
                    device=DEV, acq_optimizer_kwargs={"n_points": 600})
    opt.trace = []
    X, y = told_quadratic(opt.space, 3)
    opt.tell(X, y)
    rec = opt.trace[-1]
    assert rec["lattice"] == 6
    cand = lattice_transformed(opt.space, 600, rec["cand_seed"], DEV).cpu().numpy()
    assert np.array_equal(cand, lattice_ref(MIXED, 600, rec["cand_seed"]))
    st = oracle_state(opt)
    gp = opt.models[-1].dev
    y_opt = float(np.min(y))
    moved = 0
    for acq in ("EI", "LCB", "PI"):
        starts = cand[np.asarray(rec["top"][acq])]
        xs, fs = rec["polished"][acq]
        assert xs.shape == (5, 3) and starts.shape == (5, 3)
        assert xs[:, 1].tobytes() == starts[:, 1].tobytes()             # bit-equal to its start's
        assert np.isin(xs[:, 1], np.arange(6) / 5.0).all()
        assert (xs[:, [0, 2]] >= 0.0).all() and (xs[:, [0, 2]] <= 1.0).all()
        code = np.array([acq_code(acq)], dtype=np.int32)

        def fg(v):
            f, g = gp.acq_grad(v[None], code, y_opt)
            return float(f[0]), g[0].copy()

        for x0, x, f in zip(starts, xs, fs):
            bounds = [(0.0, 1.0), (x0[1], x0[1]), (0.0, 1.0)]
            xr, fr, _ = fmin_l_bfgs_b(fg, x0, bounds=bounds, approx_grad=False, maxiter=20)
            print(f"{acq}: x - scipy {np.max(np.abs(x - xr)):.3e}, f - scipy {abs(f - fr):.3e} of {abs(fr):.3e}")
            assert np.max(np.abs(x - xr)) <= 1e-6, (x, xr)
            assert abs(f - fr) <= 1e-9 * max(1.0, abs(fr))
            assert O.acquisition_and_grad(st, x, y_opt, acq)[0] <= O.acquisition_and_grad(st, x0, y_opt, acq)[0]
            moved += not np.array_equal(x, x0)
    assert moved > 0                                                    # the polish did something
    x = opt.ask()
    assert isinstance(x[1], (int, np.integer)) and 0 <= x[1] <= 5
    # the trained point's discrete value is the polished point's, not a rounding of something else
    pick = opt.next_xs_[rec["pick"]]
    assert x[1] == round(pick[1] * 5) and pick[1] in rec["polished"][("EI", "LCB", "PI")[rec["pick"]]][0][:, 1]


# ---- determinism -------------------------------------------------------------------------------

def test_one_seed_gives_one_batch():
    batches = []
    for _ in range(2):
        opt = Optimizer(MIXED, acq_func="EI", n_initial_points=8, random_state=11, candidates="lattice", device=DEV,
                        acq_optimizer_kwargs={"n_points": 600})
        opt.tell(*told_quadratic(opt.space, 11))
        batches.append(opt.ask(4))
    assert batches[0] == batches[1] and len(batches[0]) == 4


@pytest.mark.parametrize("dims", [MIXED, DISCRETE, [Real(0.0, 1.0), Real(0.0, 1.0)]],
                         ids=["mixed", "discrete", "reals"])
def test_one_randomstate_draw_per_proposal_as_device(dims):
    states = {}
    for source in ("lattice", "device"):
        opt = Optimizer(dims, acq_func="EI", n_initial_points=8, random_state=5, candidates=source, device=DEV,
                        acq_optimizer_kwargs={"n_points": 600})
        opt.trace = []
        opt.tell(*told_quadratic(opt.space, 5))
        states[source] = (opt.rng.get_state(), opt.trace[-1]["cand_seed"])
    (sa, ca), (sb, cb) = states["lattice"], states["device"]
    assert ca == cb and sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
