"""The topclass builders (models.test_cnn / CNNModel / topclass_space) against the
reference's text, by hand: mpiLAPI.py:178-195, base_model.py:21-55,
hyperparameter_search_option3.py:108-123.  Keras is not installed here, so the JSON is
compared with what ``Sequential.to_json()`` of those lines holds, layer by layer, not with
Keras' own output."""
import json

import pytest

from mpi_opt_amd import models as M
from mpi_opt_amd import search
from mpi_opt_amd.topclass import TopclassSpec


def layers_of(js):
    d = json.loads(js)
    assert d["class_name"] == "Sequential"
    return d["config"]["layers"]


def test_test_cnn_layers_match_the_reference():
    ls = layers_of(M.test_cnn())
    assert [l["class_name"] for l in ls] == ["Conv2D", "Conv2D", "MaxPooling2D", "Dropout", "Flatten", "Dense",
                                             "Dropout", "Dense"]
    c1, c2, pool, dr1, _, d1, dr2, d2 = (l["config"] for l in ls)
    assert c1["batch_input_shape"] == [None, 150, 94, 5] and "batch_input_shape" not in c2
    for c in (c1, c2):
        assert (c["filters"], c["kernel_size"], c["strides"], c["padding"], c["activation"]) == \
            (32, [3, 3], [3, 3], "valid", "relu")
    assert pool["pool_size"] == [2, 2] and pool["strides"] == [2, 2] and pool["padding"] == "valid"
    assert dr1["rate"] == 0.25 and dr2["rate"] == 0.5                 # dropout / 2, dropout (default 0.5)
    assert (d1["units"], d1["activation"]) == (128, "relu") and (d2["units"], d2["activation"]) == (3, "softmax")
    # the arguments: dropout and kernel_size are live, lr / llr never reach the JSON
    ls = layers_of(M.test_cnn(dropout=0.3, kernel_size=5, llr=7.0, lr=0.1))
    assert ls[0]["config"]["kernel_size"] == [5, 5] and ls[1]["config"]["kernel_size"] == [5, 5]
    assert ls[3]["config"]["rate"] == 0.15 and ls[6]["config"]["rate"] == 0.3
    assert M.test_cnn(dropout=0.3, kernel_size=5) == M.test_cnn(dropout=0.3, kernel_size=5, llr=7.0, lr=0.1)
    assert "0.1" not in M.test_cnn(dropout=0.5, lr=0.1)


# conv1, conv2 and pool outputs at 150 x 94 for k = 1 .. 9: (in - k) // 3 + 1 twice, then // 2
GEOMETRY = {1: (50, 32, 17, 11, 8, 5), 2: (50, 31, 17, 10, 8, 5), 3: (50, 31, 16, 10, 8, 5), 4: (49, 31, 16, 10, 8, 5),
            5: (49, 30, 15, 9, 7, 4), 6: (49, 30, 15, 9, 7, 4), 7: (48, 30, 14, 8, 7, 4), 8: (48, 29, 14, 8, 7, 4),
            9: (48, 29, 14, 7, 7, 3)}


@pytest.mark.parametrize("k", range(1, 10))
def test_spec_from_json_geometry(k):
    spec = M.spec_from_json(M.test_cnn(kernel_size=k, dropout=0.4), lr=2e-3, seed=9)
    assert isinstance(spec, TopclassSpec)
    assert (spec.kernel_size, spec.dropout, spec.lr, spec.seed, spec.input_shape, spec.classes) == \
        (k, 0.4, 2e-3, 9, (150, 94, 5), 3)
    g = spec.geometry()
    assert (g["H1"], g["W1"], g["H2"], g["W2"], g["Hp"], g["Wp"]) == GEOMETRY[k]
    assert g["K1"] == g["Hp"] * g["Wp"] * 32
    assert spec.param_shapes() == {"w1": (k, k, 5, 32), "b1": (32,), "w2": (k, k, 32, 32), "b2": (32,),
                                   "w3": (g["K1"], 128), "b3": (128,), "w4": (128, 3), "b4": (3,)}
    fwd = (2 * k * k * 5 * 32 * g["H1"] * g["W1"] + 2 * k * k * 32 * 32 * g["H2"] * g["W2"] + 2 * g["K1"] * 128
           + 2 * 128 * 3)
    assert spec.flops_per_sample_fwd() == fwd
    assert spec.flops_per_sample_train() == 3 * fwd - 2 * k * k * 5 * 32 * g["H1"] * g["W1"]


def test_the_issue_states_the_reference_geometry():
    assert GEOMETRY[1][:2] == (50, 32) and GEOMETRY[9][:2] == (48, 29)
    assert GEOMETRY[1][2:4] == (17, 11) and GEOMETRY[9][2:4] == (14, 7)
    assert GEOMETRY[1][4:] == (8, 5) and GEOMETRY[9][4:] == (7, 3)


def _variant(edit):
    d = json.loads(M.test_cnn())
    edit(d["config"]["layers"])
    return json.dumps(d)


@pytest.mark.parametrize("edit", [
    lambda ls: ls[0]["config"].update(strides=[1, 1]),
    lambda ls: ls[1]["config"].update(strides=[2, 2]),
    lambda ls: ls[0]["config"].update(filters=16),
    lambda ls: ls[1]["config"].update(padding="same"),
    lambda ls: ls[1]["config"].update(kernel_size=[5, 5]),
    lambda ls: ls[0]["config"].update(kernel_size=[3, 2]),
    lambda ls: ls[0]["config"].update(activation="tanh"),
    lambda ls: ls[2]["config"].update(pool_size=[3, 3], strides=[3, 3]),
    lambda ls: ls[5]["config"].update(units=64),
    lambda ls: ls[3]["config"].update(rate=0.5),
    lambda ls: ls[0]["config"].update(batch_input_shape=[None, 150, 94, 9]),
    lambda ls: ls[0]["config"].update(batch_input_shape=[None, 17, 94, 5]),      # conv2 output 1 on H at k = 3
    lambda ls: ls[7]["config"].update(units=1),
    lambda ls: ls.pop(3),
], ids=lambda f: None)
def test_spec_from_json_refuses_variants(edit):
    with pytest.raises(ValueError):
        M.spec_from_json(_variant(edit))


def test_kernel_sizes_outside_the_engine_are_refused():
    for k in (0, 10):
        with pytest.raises(ValueError):
            M.spec_from_json(M.test_cnn(kernel_size=k))
    with pytest.raises(ValueError):
        TopclassSpec(loss="mse").options()


def test_cnn_model():
    m = M.CNNModel()
    assert isinstance(m, M.BaseModel) and m.get_name() == "CNN_model"
    assert m.get_parameter_grid() == [(3, 9), (.0, .5), (-5, 1)]
    spec = M.spec_from_json(m.build([7, 0.2, -3.0]), lr=1e-3)
    assert (spec.kernel_size, spec.dropout, spec.input_shape, spec.classes) == (7, 0.2, (150, 94, 5), 3)
    assert m.build([7, 0.2, -3.0]) == m.build([7, 0.2, 0.5])           # the lr dimension is compiled away
    assert M.spec_from_json(M.CNNModel(input_shape=(60, 40, 2)).build([3, 0.0, -3])).input_shape == (60, 40, 2)


def test_topclass_space_and_builder():
    from mpi_opt_amd.space import Integer, Real

    sp = M.topclass_space()
    assert [p.name for p in sp] == ["dropout", "kernel_size", "llr"]
    assert isinstance(sp[0], Real) and isinstance(sp[1], Integer) and isinstance(sp[2], Real)
    assert [(p.low, p.high) for p in sp] == [(0.0, 1.0), (1, 6), (1.0, 10.0)]
    spec = M.BuilderFromFunction(M.test_cnn, sp).builder(0.3, 4, 5.0).spec()
    assert (spec.kernel_size, spec.dropout, spec.lr) == (4, 0.3, 1e-3)       # llr is dead: the trainer's lr
    assert spec.geometry()["K1"] == 8 * 5 * 32


def test_other_topologies_ingest_as_before():
    from mpi_opt_amd.population import TrialSpec

    s = M.spec_from_json(M.test_mnist(nb_filters=20, kernel_size=4, pool_size=3, dense=77), lr=2e-3, seed=5)
    assert isinstance(s, TrialSpec)
    assert (s.nb_filters, s.kernel_size, s.pool_size, s.dense, s.lr, s.dropout, s.seed) == (20, 4, 3, 77, 2e-3, 0.25, 5)
    d = M.spec_from_json(M.test_densenet(img_dim=(32, 32, 3), nb_classes=10), lr=3e-3)
    assert isinstance(d, M.DenseNetSpec) and d.lr == 3e-3 and d.arch.img_dim == (32, 32, 3)
    with pytest.raises(ValueError):
        M.spec_from_json(json.dumps({"class_name": "Graph", "config": {}}))


def test_cli_wiring(capsys):
    p = search.make_parser()
    args = p.parse_args(["--example", "topclass"])
    prov = search.example_provider(args.example)
    assert prov.model_fn is M.test_cnn and [q.name for q in prov.parameters] == ["dropout", "kernel_size", "llr"]
    assert search.example_provider("mnist").model_fn is M.test_mnist
    assert search.EXAMPLE_DATASETS["topclass"] == ("Images", "Labels")
    small = search.example_provider("topclass", (30, 26, 5)).builder(0.5, 2, 3.0).spec()
    assert small.input_shape == (30, 26, 5)
    cost = search.modelled_cost_fn(prov)
    assert cost([0.5, 3, 3.0]) == prov.builder(0.5, 3, 3.0).spec().flops_per_sample_train() * 1e-9
    helps = {a.dest: a.help or "" for a in p._actions}
    assert "topclass" in helps["n_samples"] and "Images" in helps["data_dir"]
    assert search.main(["--example", "gan"]) == 2
    assert "3D GAN" in capsys.readouterr().err
    with pytest.raises(ValueError):
        search.example_provider("gan")
