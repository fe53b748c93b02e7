"""Model-builder plugin interface, drop-in for the reference's builders.

* ``test_mnist(**args) -> str`` -- /root/reference/mpiLAPI.py:138-176: the Keras
  MNIST ConvNet as a JSON string.  Keras is not available (nor needed): the
  JSON mirrors ``Sequential.to_json()`` (``class_name``/``config``/``layers``) and
  is what :func:`spec_from_json` ingests into a device :class:`TrialSpec`.
  The reference reads ``args.get('drop_out', 0.25)`` while its search space
  names the dimension ``dropout`` (option3:131): the dimension is dead and
  the rate stays 0.25 -- reproduced here.
* ``test_densenet`` -- mpiLAPI.py:197-201 (DenseNet) as a JSON spec that
  ingests into a :class:`DenseNetSpec` the DenseNet population engine
  (densenet.py) trains.
* ``test_cnn`` -- mpiLAPI.py:178-195, the strided CNN of option3's ``topclass``
  example (option3:108-123), as the Sequential JSON that ingests into a
  :class:`~mpi_opt_amd.topclass.TopclassSpec` (topclass.py trains it); ``CNNModel``
  (base_model.py:21-55) builds the same network.  Here ``dropout`` and
  ``kernel_size`` are live; ``lr`` / ``llr`` are compiled into the model, which
  ``to_json`` drops.  The 3-D GAN (option3:144-168) stays out of scope.
* ``BuilderFromFunction`` -- hyperparameter_search_option3.py:22-31: zips the
  named dimensions with a parameter list, calls ``model_fn(**named)`` and wraps
  the JSON in a ``ModelFromJson`` with settable ``comm`` / ``device`` and
  ``get_device_name`` (used by process_block.py:64-67).
* ``BaseModel`` / ``CNNModel`` / ``DenseNetModel`` -- base_model.py:8-19, 21-55, 57-92:
  ``build(params) -> json``, ``get_parameter_grid()``, ``get_name()``.
"""
from __future__ import annotations

import json

import numpy as np

from .population import TrialSpec

KERAS_VERSION = "2.2.4"   # what the JSON claims to be; the content is all that is read


def _layer(cls, **cfg):
    return {"class_name": cls, "config": cfg}


def _sequential(layers, name="sequential_1"):
    return json.dumps({"class_name": "Sequential", "config": {"name": name, "layers": layers},
                       "keras_version": KERAS_VERSION, "backend": "tensorflow"})


def test_mnist(**args):
    """MNIST ConvNet from keras/examples/mnist_cnn.py (mpiLAPI.py:138-176)."""
    nb_classes = 10
    nb_filters = int(args.get("nb_filters", 32))
    ps = int(args.get("pool_size", 2))
    ks = int(args.get("kernel_size", 3))
    do = float(args.get("drop_out", 0.25))      # sic: the space's 'dropout' never reaches here
    dense = int(args.get("dense", 128))
    layers = [
        _layer("Conv2D", name="conv2d_1", filters=nb_filters, kernel_size=[ks, ks], strides=[1, 1],
               padding="valid", batch_input_shape=[None, 28, 28, 1], data_format="channels_last",
               activation="linear", use_bias=True, kernel_initializer="glorot_uniform",
               bias_initializer="zeros"),
        _layer("Activation", name="activation_1", activation="relu"),
        _layer("Conv2D", name="conv2d_2", filters=nb_filters, kernel_size=[ks, ks], strides=[1, 1],
               padding="valid", activation="linear", use_bias=True, kernel_initializer="glorot_uniform",
               bias_initializer="zeros"),
        _layer("Activation", name="activation_2", activation="relu"),
        _layer("MaxPooling2D", name="max_pooling2d_1", pool_size=[ps, ps], strides=[ps, ps], padding="valid"),
        _layer("Dropout", name="dropout_1", rate=do),
        _layer("Flatten", name="flatten_1"),
        _layer("Dense", name="dense_1", units=dense, activation="linear", use_bias=True,
               kernel_initializer="glorot_uniform", bias_initializer="zeros"),
        _layer("Activation", name="activation_3", activation="relu"),
        _layer("Dropout", name="dropout_2", rate=do),
        _layer("Dense", name="dense_2", units=nb_classes, activation="linear", use_bias=True,
               kernel_initializer="glorot_uniform", bias_initializer="zeros"),
        _layer("Activation", name="activation_4", activation="softmax"),
    ]
    return _sequential(layers)


def test_cnn(**args):
    """mpiLAPI.py:178-195: two strided valid convolutions, a 2x2 max-pool and two dense
    layers on 150x94x5 images, activations inside the layers (8 layers).  ``lr`` /
    ``llr`` are read as the reference reads them and, compiled into the optimizer that
    ``to_json`` drops, never reach the JSON.  ``input_shape`` (an addition; the reference
    fixes 150x94x5) builds the same network on other images."""
    return _cnn_json(args.get("dropout", 0.5), args.get("kernel_size", 3), args.get("input_shape", (150, 94, 5)),
                     lr=args.get("lr", np.exp(-args.get("llr", np.log(1. / 1e-3)))))


def _cnn_json(dropout, kernel_size, input_shape, lr=None, nb_classes=3):
    do, ks = float(dropout), int(kernel_size)
    conv = dict(filters=32, kernel_size=[ks, ks], strides=[3, 3], padding="valid", data_format="channels_last",
                activation="relu", use_bias=True, kernel_initializer="glorot_uniform", bias_initializer="zeros")
    dense = dict(use_bias=True, kernel_initializer="glorot_uniform", bias_initializer="zeros")
    layers = [
        _layer("Conv2D", name="conv2d_1", batch_input_shape=[None] + [int(v) for v in input_shape], **conv),
        _layer("Conv2D", name="conv2d_2", **conv),
        _layer("MaxPooling2D", name="max_pooling2d_1", pool_size=[2, 2], strides=[2, 2], padding="valid"),
        _layer("Dropout", name="dropout_1", rate=do / 2),
        _layer("Flatten", name="flatten_1"),
        _layer("Dense", name="dense_1", units=128, activation="relu", **dense),
        _layer("Dropout", name="dropout_2", rate=do),
        _layer("Dense", name="dense_2", units=nb_classes, activation="softmax", **dense),
    ]
    return _sequential(layers)


def test_densenet(nb_classes=3, img_dim=(150, 94, 5), depth=10, nb_dense_block=3, growth_rate=12,
                  dropout_rate=0.00, nb_filter=16, lr=1e-3):
    """mpiLAPI.py:197-201: ``DenseNet(...)`` (densenet.py:135-196), compiled with
    ``Adam(lr)``, returned as ``to_json()`` -- the Keras functional-model JSON
    (:func:`mpi_opt_amd.keras_json.densenet_json`).  ``to_json`` carries no
    compile arguments, so ``lr`` does not reach the trainer (as in the reference)."""
    from .keras_json import densenet_json

    return densenet_json(nb_classes, img_dim, depth, nb_dense_block, growth_rate, nb_filter,
                         dropout_rate=dropout_rate)


class DenseNetSpec:
    """A DenseNet trial: the architecture (densenet.py:135) and its Adam lr, which
    the reference compiles into the model (base_model.py:67-71) and searches."""

    def __init__(self, arch, lr):
        self.arch = arch
        self.lr = float(lr)

    def flops_per_sample_train(self):
        from .densenet import flops_per_sample_train

        return flops_per_sample_train(self.arch.layers())


def spec_from_json(json_str, lr=1e-3, seed=0):
    """Ingest a Keras JSON into a device spec: the test_mnist Sequential topology
    -> :class:`TrialSpec`; a functional DenseNet ``Model`` (densenet.py's graph,
    from ``test_densenet`` / ``DenseNetModel.build`` or Keras itself) ->
    :class:`DenseNetSpec` trained with the trainer's ``lr``."""
    d = json.loads(json_str)
    if d.get("class_name") in ("Model", "Functional"):
        from .keras_json import densenet_arch_from_json

        arch, wd = densenet_arch_from_json(d)
        if abs(wd - 1e-4) > 1e-10:
            raise ValueError(f"DenseNet population trains weight_decay 1e-4 (densenet.py:136), JSON has {wd}")
        return DenseNetSpec(arch, lr)
    if d.get("class_name") != "Sequential":
        raise ValueError("population engines train the test_mnist / test_cnn Sequential topologies and the "
                         "functional DenseNet only")
    layers = d["config"]["layers"] if isinstance(d["config"], dict) else d["config"]
    kinds = [l["class_name"] for l in layers]
    if kinds == _CNN_KINDS:
        return _topclass_spec(layers, lr, seed)
    expect = ["Conv2D", "Activation", "Conv2D", "Activation", "MaxPooling2D", "Dropout", "Flatten", "Dense",
              "Activation", "Dropout", "Dense", "Activation"]
    if kinds != expect:
        raise ValueError(f"unsupported topology {kinds}")
    c1, c2, pool, dr1, d1, dr2, d2 = (layers[i]["config"] for i in (0, 2, 4, 5, 7, 9, 10))
    F, k = int(c1["filters"]), int(c1["kernel_size"][0])
    shape = c1.get("batch_input_shape", [None, 28, 28, 1])
    if list(shape[1:]) != [28, 28, 1] or c1.get("padding", "valid") != "valid":
        raise ValueError("population engine expects 28x28x1 inputs and valid convolutions")
    if int(c2["filters"]) != F or int(c2["kernel_size"][0]) != k or int(d2["units"]) != 10:
        raise ValueError("unsupported test_mnist variant")
    if float(dr1["rate"]) != float(dr2["rate"]):
        raise ValueError("both dropout layers must share one rate")
    acts = [layers[i]["config"]["activation"] for i in (1, 3, 8, 11)]
    if acts != ["relu", "relu", "relu", "softmax"]:
        raise ValueError(f"unsupported activations {acts}")
    return TrialSpec(nb_filters=F, kernel_size=k, pool_size=int(pool["pool_size"][0]), dense=int(d1["units"]),
                     lr=lr, dropout=float(dr1["rate"]), seed=seed)


_CNN_KINDS = ["Conv2D", "Conv2D", "MaxPooling2D", "Dropout", "Flatten", "Dense", "Dropout", "Dense"]


def _pair(v):
    return [int(v), int(v)] if np.isscalar(v) else [int(t) for t in v]


def _topclass_spec(layers, lr, seed):
    """The test_cnn topology (mpiLAPI.py:178-195) -> TopclassSpec; its variants are refused."""
    from .topclass import DENSE, FILTERS, TopclassSpec

    c1, c2, pool, dr1, _, d1, dr2, d2 = (l["config"] for l in layers)
    shape = c1.get("batch_input_shape")
    if shape is None or len(shape) != 4:
        raise ValueError("test_cnn topology without a [None, H, W, C] batch_input_shape")
    k = _pair(c1["kernel_size"])
    for c in (c1, c2):
        if _pair(c["kernel_size"]) != k or k[0] != k[1]:
            raise ValueError(f"unsupported test_cnn variant: kernel sizes {c1['kernel_size']} / {c2['kernel_size']}")
        if _pair(c.get("strides", 1)) != [3, 3] or c.get("padding", "valid") != "valid":
            raise ValueError("unsupported test_cnn variant: the population engine trains strides 3, valid padding")
        if int(c["filters"]) != FILTERS or c.get("activation") != "relu":
            raise ValueError(f"unsupported test_cnn variant: {FILTERS} relu filters per convolution")
        if c.get("data_format", "channels_last") != "channels_last" or _pair(c.get("dilation_rate", 1)) != [1, 1]:
            raise ValueError("unsupported test_cnn variant: channels_last, undilated convolutions")
    if _pair(pool["pool_size"]) != [2, 2] or _pair(pool.get("strides") or pool["pool_size"]) != [2, 2] \
            or pool.get("padding", "valid") != "valid":
        raise ValueError("unsupported test_cnn variant: 2x2 valid max-pool")
    if int(d1["units"]) != DENSE or d1.get("activation") != "relu" or d2.get("activation") != "softmax":
        raise ValueError(f"unsupported test_cnn variant: Dense({DENSE}, relu) -> Dense(classes, softmax)")
    rate = float(dr2["rate"])
    if float(dr1["rate"]) != rate / 2:
        raise ValueError("unsupported test_cnn variant: the first dropout rate is half the second")
    spec = TopclassSpec(kernel_size=k[0], dropout=rate, lr=lr, seed=seed, input_shape=tuple(int(v) for v in shape[1:]),
                        classes=int(d2["units"]))
    spec.geometry()   # refuses shapes the kernels do not take
    return spec


class ModelFromJson:
    """Stand-in for mpi_learn's ModelFromJsonTF (option3:27-31)."""

    def __init__(self, comm, json_str=None, device_name="cpu"):
        self.comm = comm
        self.json_str = json_str
        self.device = device_name

    def get_device_name(self, device):
        return device

    def spec(self, lr=1e-3, seed=0):
        return spec_from_json(self.json_str, lr=lr, seed=seed)


class BuilderFromFunction:
    """option3:22-31: builder(*params) -> ModelFromJson(model_fn(**named params))."""

    def __init__(self, model_fn, parameters):
        self.model_fn = model_fn
        self.parameters = parameters

    def builder(self, *params):
        args = dict(zip([p.name for p in self.parameters], params))
        return ModelFromJson(None, json_str=self.model_fn(**args))


class BaseModel:
    """base_model.py:8-19 interface."""

    def build(self, params):
        raise NotImplementedError

    def get_parameter_grid(self):
        raise NotImplementedError

    def get_name(self):
        raise NotImplementedError


class CNNModel(BaseModel):
    """base_model.py:21-55: test_cnn's network on ``input_shape``, 3 classes."""

    def __init__(self, input_shape=(150, 94, 5)):
        self.input_shape = input_shape

    def build(self, params):
        """base_model.py:26-45: the lr dimension (10**params[2]) is compiled into the
        model, which ``to_json`` drops.  The reference builds a functional ``Model``
        whose ``Flatten(x)`` cannot run; the network it means is test_cnn's, returned
        as that Sequential JSON."""
        return _cnn_json(float(params[1]), int(params[0]), self.input_shape, lr=10.0 ** params[2])

    def get_parameter_grid(self):
        return [(3, 9), (.0, .5), (-5, 1)]

    def get_name(self):
        return "CNN_model"


class DenseNetModel(BaseModel):
    """base_model.py:57-92."""

    def __init__(self, input_shape=(150, 94, 5)):
        self.input_shape = input_shape

    def build(self, params):
        """base_model.py:62-73: the lr dimension (10**params[5]) is compiled into the
        model, which ``to_json`` drops -- the JSON carries the architecture only."""
        return test_densenet(nb_classes=3, img_dim=self.input_shape, depth=int(params[0]),
                             nb_dense_block=int(params[1]), growth_rate=int(params[2]), dropout_rate=float(params[3]),
                             nb_filter=int(params[4]), lr=10.0 ** params[5])

    def get_parameter_grid(self):
        return [(10, 10), (3, 3), (12, 12), (.0, .0), (16, 16), (-5, 1)]

    def get_name(self):
        return "DenseNet"


# --- search spaces of the reference examples --------------------------------
def mnist_space():
    """option3:126-133."""
    from .space import Integer, Real

    return [Integer(10, 50, name="nb_filters"), Integer(2, 10, name="pool_size"),
            Integer(2, 10, name="kernel_size"), Integer(50, 200, name="dense"),
            Real(0.0, 1.0, name="dropout")]


def topclass_space():
    """option3:111-113."""
    from .space import Integer, Real

    return [Real(0.0, 1.0, name="dropout"), Integer(1, 6, name="kernel_size"), Real(1., 10., name="llr")]


def flops_of_params(model_fn, names, params):
    spec = spec_from_json(model_fn(**dict(zip(names, params))))
    return spec.flops_per_sample_train()


__all__ = ["test_mnist", "test_cnn", "test_densenet", "spec_from_json", "DenseNetSpec", "ModelFromJson",
           "BuilderFromFunction", "BaseModel", "CNNModel", "DenseNetModel", "mnist_space", "topclass_space"]
