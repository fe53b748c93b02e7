"""``mpo_space_sample`` on the GPU against its numpy restatement (tests/philox_ref.py):
the law is fixed by include/mpo.h, so every comparison is ``np.array_equal`` -- no
tolerance."""
import numpy as np
import pytest
import torch

from mpi_opt_amd import _lib
from mpi_opt_amd.candidates import dim_table, sample_transformed
from mpi_opt_amd.models import mnist_space
from mpi_opt_amd.space import Categorical, Integer, Real, Space
from tests import philox_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = (0x9E3779B9 << 32) | 0x12345                 # both key words in use
SIZES = (1, 63, 64, 65, 1000, 4097)
WRAP = 2 ** 32 - 3                                  # with m = 8 the rows cross the counter's word boundary

SPACES = {
    "mnist": mnist_space(),                         # d = 5, odd
    # 7 dimensions, 9 columns, the last Philox pair half used
    "mixed": [Real(1e-3, 1.0, prior="log-uniform"), Integer(4, 4), Integer(0, 1), Categorical("ab"),
              Categorical("abc"), Categorical("a"), Real(-2.0, 2.0)],
    "reals32": [Real(0.0, 1.0) for _ in range(32)],
    "integer": [Integer(3, 9)],
}
_REF = {}


def ref(name, m, first=0, seed=SEED):
    """Rows [first, first + m) of the reference set; the low rows are computed once per space."""
    if first + m <= SIZES[-1] + 5:
        key = (name, seed)
        if key not in _REF:
            _REF[key] = P.sample_transformed(SPACES[name], SIZES[-1] + 5, seed)
            _REF[key].setflags(write=False)
        return _REF[key][first:first + m]
    return P.sample_transformed(SPACES[name], m, seed, first=first)


def device(name, m, first=0, seed=SEED):
    return sample_transformed(Space(SPACES[name]), m, seed, DEV, first=first).cpu().numpy()


@pytest.mark.parametrize("name", list(SPACES))
def test_rows_equal_the_reference_bits(name):
    d = Space(SPACES[name]).transformed_n_dims
    assert d == {"mnist": 5, "mixed": 9, "reals32": 32, "integer": 1}[name]
    for first in (0, 5):
        for m in SIZES:
            got = device(name, m, first)
            assert got.shape == (m, d) and got.dtype == np.float64
            assert np.array_equal(got, ref(name, m, first)), (name, m, first)
    assert np.array_equal(device(name, 8, WRAP), ref(name, 8, WRAP))
    assert not np.array_equal(ref(name, 8, WRAP)[:3], ref(name, 8, WRAP)[3:6])


@pytest.mark.parametrize("name", ["mnist", "mixed"])
def test_split_invariance(name):
    m = 1000
    whole = device(name, m)
    for a in (1, 64, 777):
        parts = np.concatenate([device(name, a), device(name, m - a, first=a)])
        assert np.array_equal(parts, whole), a


def test_repeatable_and_seed_dependent():
    a, b = device("mixed", 1000), device("mixed", 1000)
    assert np.array_equal(a, b)
    other = device("mixed", 1000, seed=SEED + 1)
    assert np.array_equal(other, ref("mixed", 1000, seed=SEED + 1))
    assert not (other == a).all(axis=1).any()       # column 0 is a 53-bit Real: no row repeats
    high = device("mixed", 1000, seed=SEED + (1 << 32))
    assert np.array_equal(high, ref("mixed", 1000, seed=SEED + (1 << 32))) and not np.array_equal(high, a)


def test_no_rows():
    out = sample_transformed(Space(SPACES["mnist"]), 0, SEED, DEV)
    assert tuple(out.shape) == (0, 5)
    table, d = dim_table(Space(SPACES["mnist"]))
    assert _lib.lib().mpo_space_sample(table, len(table), d, SEED, 7, 0, None, _lib.stream_handle(DEV)) == 0


def test_second_pass_with_a_pair_count_that_divides_the_grid():
    """32 Reals x 40 000 rows: 640 000 (row, pair) items, more than the capped grid's 2^19
    threads, so some threads take a second item.  16 pairs divide 2^19: the stride moves
    the row only (sr = 0), the pair carry does not run here (the next test's does)."""
    m = 40_000
    assert np.array_equal(device("reals32", m, first=11), P.sample_transformed(SPACES["reals32"], m, SEED, first=11))


REALS10 = [Real(0.0, 1.0) for _ in range(10)]


REALS13 = [Real(0.0, 1.0) for _ in range(13)]


@pytest.mark.parametrize("dims, m, first, passes", [
    (SPACES["mnist"], 200_000, 7, 2),                   # 3 pairs: stride 2^19 = 174762 * 3 + 2
    (REALS10, 110_000, 3, 2),                           # 5 pairs: stride 2^19 = 104857 * 5 + 3
    (REALS13, 80_000, 0, 2),                            # 7 pairs, the last half used: 74898 * 7 + 2
    (SPACES["mnist"], 450_000, 2 ** 32 - 200_000, 3),   # the carry twice per thread, across the counter word
], ids=["mnist-200k", "reals10-110k", "reals13-80k", "mnist-450k-wrap"])
def test_stride_carry_over_several_passes(dims, m, first, passes):
    """More (row, pair) items than the capped grid's 2^19 threads with a pair count that
    does not divide it: a thread's later items move by (sq rows, sr pairs) and the pair
    index wraps into the next row.  Every row must be written once, with its own bits."""
    n_pairs = (len(dims) + 1) // 2
    assert -(-m * n_pairs // 2 ** 19) == passes
    got = sample_transformed(Space(dims), m, SEED, DEV, first=first).cpu().numpy()
    assert np.array_equal(got, P.sample_transformed(dims, m, SEED, first=first))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name, m", [("mnist", 65), ("mnist", 64), ("integer", 1), ("mixed", 4097)])
def test_writes_stay_inside_an_output_at_either_alignment(name, m, offset):
    """The ABI on a buffer that is 16 B aligned (offset 0) or only 8 B aligned (offset 1),
    with guard words on both sides."""
    table, d = dim_table(Space(SPACES[name]))
    guard = 4
    buf = torch.full((guard + offset + m * d + guard,), -7.0, dtype=torch.float64, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lo = guard + offset
    _lib.check(_lib.lib().mpo_space_sample(table, len(table), d, SEED, 5, m, buf.data_ptr() + 8 * lo,
                                           _lib.stream_handle(DEV)), "mpo_space_sample")
    host = buf.cpu().numpy()
    assert np.array_equal(host[lo:lo + m * d].reshape(m, d), ref(name, m, 5))
    assert (host[:lo] == -7.0).all() and (host[lo + m * d:] == -7.0).all()
