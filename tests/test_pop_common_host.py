"""What the three population engines share on the Python side (no GPU): one
``glorot_uniform_init``, one ``options()``, one base class with the step methods."""
import hashlib
import itertools

import pytest

from mpi_opt_amd import _lib, densenet, population, topclass
from mpi_opt_amd.population import TrialSpec
from mpi_opt_amd.topclass import TopclassSpec

# SHA-256 of what commit cb287160bba3's two functions, population.glorot_uniform_init and
# topclass.glorot_uniform_init, return at seed 11 (name, shape, dtype and bytes of every tensor)
MNIST_INIT = "bc1b469f2ba033e46e5f5900850c9f663f4fc7763c13425f7c5814702d9861b8"
TOPCLASS_INIT = "16fbdff090ab79e70f7058e108f9bb0d0741e8a82f260d46cd7bc2fbe55447d3"


def digest(params):
    h = hashlib.sha256()
    for name, v in params.items():
        for part in (name.encode(), str(v.shape).encode(), str(v.dtype).encode(), v.tobytes()):
            h.update(part)
    return h.hexdigest()


def test_one_init_draws_what_the_two_drew():
    assert topclass.glorot_uniform_init is population.glorot_uniform_init
    init = population.glorot_uniform_init
    assert digest(init(TrialSpec(nb_filters=5, kernel_size=3, dense=7), 11)) == MNIST_INIT
    assert digest(init(TopclassSpec(kernel_size=2, input_shape=(21, 17, 5), classes=3), 11)) == TOPCLASS_INIT


def test_options_bits_agree_and_refuse_the_unknown():
    for loss, opt in itertools.product(_lib.LOSS_CODES, _lib.OPT_CODES):
        bits = _lib.LOSS_CODES[loss] | _lib.OPT_CODES[opt]
        assert TrialSpec(loss=loss, optimizer=opt).options() == bits
        assert TopclassSpec(loss=loss, optimizer=opt).options() == bits
    for spec in (TrialSpec, TopclassSpec):
        with pytest.raises(ValueError, match="unsupported loss / optimizer"):
            spec(loss="hinge").options()
        with pytest.raises(ValueError, match="unsupported loss / optimizer"):
            spec(optimizer="rmsprop").options()


def test_engines_share_the_base_and_its_step_methods():
    engines = (population.PopulationEngine, topclass.TopclassPopulation, densenet.DenseNetPopulation)
    base = population._PopulationBase
    assert all(issubclass(e, base) for e in engines)
    for name in ("train_step", "eval_step", "eval_reset", "reset_optimizer", "__del__", "fit_folds"):
        assert all(getattr(e, name) is getattr(base, name) for e in engines), name
    assert sorted({e._C for e in engines}) == ["mpo_dn", "mpo_pop", "mpo_tc"]
    # the flat-arena layer is the MNIST and topclass engines' alone
    flat = population._FlatArenaPopulation
    assert issubclass(engines[0], flat) and issubclass(engines[1], flat) and not issubclass(engines[2], flat)
    for name in ("set_params", "get_params", "get_grads", "activation"):
        assert getattr(engines[0], name) is getattr(engines[1], name) is getattr(flat, name), name
    # retiring members: MNIST and DenseNet have it, topclass does not (train_folds looks for it)
    assert engines[0].set_active is engines[2].set_active and engines[0].step_work is engines[2].step_work
    assert not hasattr(engines[1], "set_active") and not hasattr(engines[1], "step_work")
