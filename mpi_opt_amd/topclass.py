"""Device-resident population of the strided ``test_cnn`` (option3's ``topclass`` example).

Replaces the per-block Keras training of ``test_cnn`` (mpiLAPI.py:178-195,
built by hyperparameter_search_option3.py:108-114; ``CNNModel`` base_model.py:21-55) the
way population.py replaces test_mnist's: every (trial, fold) pair is a member, all of
them step together through ``libmpo.so`` (csrc/topclass.hip).  The network, channels-last:

    Conv2D(32, k, strides 3, valid, relu) -> Conv2D(32, k, strides 3, valid, relu)
    -> MaxPool 2x2 -> Dropout(dropout / 2) -> Flatten -> Dense(128, relu) -> Dropout(dropout)
    -> Dense(classes, softmax)

``kernel_size`` and ``dropout`` are live hyper-parameters here (``kernel_size`` changes the
geometry of both convolutions); ``lr`` is the trainer's (``to_json`` drops the compiled
optimizer, so the builder's ``llr`` is dead).  A dropout rate outside (0, 1) is the
identity, as Keras 2's ``Dropout.call``: the space's bound ``dropout = 1.0`` trains with
rate 0.5 after the pool and no dropout after the dense layer.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import _lib
from .population import PARAM_NAMES, _FlatArenaPopulation, glorot_uniform_init, spec_options  # noqa: F401 (re-exported)

FILTERS = 32
DENSE = 128
STRIDE = 3
ACT_NAMES = ("a1", "a2", "pd", "am", "h", "hd", "z3", "dz3", "dh", "dp", "dz2", "dz1")


@dataclass
class TopclassSpec:
    """One test_cnn trial (mpiLAPI.py:178-195; space option3:111-113)."""

    kernel_size: int = 3
    dropout: float = 0.5
    lr: float = 1e-3
    seed: int = 0
    input_shape: tuple = (150, 94, 5)
    classes: int = 3
    loss: str = "categorical_crossentropy"   # what the builder compiles (mpiLAPI.py:193)
    optimizer: str = "adam"

    options = spec_options

    def geometry(self):
        """Output sizes of the two strided valid convolutions ((in - k) // 3 + 1 per axis)
        and the floor-mode pool; ValueError outside what csrc/topclass.hip accepts."""
        H, W, C = (int(v) for v in self.input_shape)
        k = int(self.kernel_size)
        if not (1 <= k <= 9):
            raise ValueError(f"kernel_size {k} outside 1..9")
        if not (1 <= C <= 8 and 1 <= H <= 256 and 1 <= W <= 256):
            raise ValueError(f"input shape {H} x {W} x {C} outside H, W 1..256, C 1..8")
        if not (2 <= int(self.classes) <= 16):
            raise ValueError(f"{self.classes} classes outside 2..16")
        out = lambda n: (n - k) // STRIDE + 1 if n >= k else 0
        H1, W1 = out(H), out(W)
        H2, W2 = out(H1), out(W1)
        if H2 < 2 or W2 < 2:
            raise ValueError(f"kernel_size {k} on {H} x {W}: conv2 output {H2} x {W2} is below 2 x 2")
        Hp, Wp = H2 // 2, W2 // 2
        return dict(H=H, W=W, C=C, k=k, H1=H1, W1=W1, H2=H2, W2=W2, Hp=Hp, Wp=Wp, K1=Hp * Wp * FILTERS)

    def param_shapes(self):
        g = self.geometry()
        k = g["k"]
        return {"w1": (k, k, g["C"], FILTERS), "b1": (FILTERS,), "w2": (k, k, FILTERS, FILTERS), "b2": (FILTERS,),
                "w3": (g["K1"], DENSE), "b3": (DENSE,), "w4": (DENSE, int(self.classes)), "b4": (int(self.classes),)}

    def flops_per_sample_fwd(self):
        g = self.geometry()
        k = g["k"]
        return (2 * k * k * g["C"] * FILTERS * g["H1"] * g["W1"] + 2 * k * k * FILTERS * FILTERS * g["H2"] * g["W2"]
                + 2 * g["K1"] * DENSE + 2 * DENSE * int(self.classes))

    def flops_per_sample_train(self):
        """Forward + input gradient + weight gradient of every layer, minus conv1's
        input gradient (never computed)."""
        g = self.geometry()
        return 3 * self.flops_per_sample_fwd() - 2 * g["k"] ** 2 * g["C"] * FILTERS * g["H1"] * g["W1"]


class TopclassPopulation(_FlatArenaPopulation):
    """A population of test_cnn members on one input shape, resident on one GPU.
    The ``PopulationEngine`` surface without ``set_active``: a stopping rule still ends
    members' histories, the stopped members keep stepping (``train_folds``), and
    ``fit_folds``' ``retire_stopped`` changes nothing.  :meth:`activation`'s pool argmax
    ``am`` is int32 (2 dy + dx)."""

    _C = "mpo_tc"
    ACT_NAMES = ACT_NAMES

    def __init__(self, specs, batch=100, device=None, init=None, init_seed=0):
        self.specs = [s if isinstance(s, TopclassSpec) else TopclassSpec(**s) for s in specs]
        if not self.specs:
            raise ValueError("TopclassPopulation: no members")
        s0 = self.specs[0]
        self.input_shape = tuple(int(v) for v in s0.input_shape)
        self.classes = int(s0.classes)
        for s in self.specs:
            if tuple(int(v) for v in s.input_shape) != self.input_shape or int(s.classes) != self.classes:
                raise ValueError("TopclassPopulation: members must share the input shape and the class count")
            if not math.isfinite(float(s.dropout)) or not float(s.lr) > 0:
                raise ValueError(f"TopclassPopulation: lr {s.lr} / dropout {s.dropout}")
            s.geometry()
        arr = (_lib.MpoTcSpec * len(self.specs))()
        for i, s in enumerate(self.specs):
            arr[i] = _lib.MpoTcSpec(int(s.kernel_size), float(s.lr), float(s.dropout), int(s.seed) & 0xFFFFFFFF,
                                    s.options())
        self._create(len(self.specs), batch, device, arr, *self.input_shape, self.classes)
        self._bind(init, init_seed)

    def _check(self, x, labels, order, row0):
        if tuple(x.shape[1:]) != self.input_shape or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"x must be contiguous float32 [n, {self.input_shape}], got {tuple(x.shape)} {x.dtype}")
        if labels.dtype != torch.int32 or labels.shape[0] != x.shape[0] or order.dtype != torch.int32:
            raise ValueError("labels [n] and order [n_members, L] must be int32")
        if order.dim() != 2 or order.shape[0] != self.n or not order.is_contiguous() or row0 < 0 \
                or row0 + self.batch > order.shape[1]:
            raise ValueError(f"order {tuple(order.shape)} does not hold rows [{row0}, {row0 + self.batch}) of "
                             f"{self.n} members")


def synthetic_topclass(n, shape=(150, 94, 5), classes=3, seed=0, device=None, labels="uniform"):
    """LCD-jet-shape synthetic data: x ~ U[0,1] f32 [n,H,W,C] (NHWC) generated on device.
    ``labels="uniform"``: uniform in [0, classes) (nothing to learn).  ``"learnable"``: the
    argmax of a fixed random linear teacher over the image average-pooled to at most 8 x 8
    cells per channel, centred at 0.5 (as ``synthetic_mnist``)."""
    dev = torch.device(device if device is not None else "cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    H, W, C = (int(v) for v in shape)
    x = torch.rand((n, H, W, C), generator=g, device=dev, dtype=torch.float32)
    y = torch.randint(0, classes, (n,), generator=g, device=dev, dtype=torch.int32)
    if labels == "learnable":
        ph, pw = min(8, H), min(8, W)
        pooled = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), (ph, pw)).reshape(n, -1) - 0.5
        w = torch.randn(pooled.shape[1], classes, generator=g, device=dev, dtype=torch.float32)
        y = torch.argmax(pooled @ w, dim=1).to(torch.int32)
    elif labels != "uniform":
        raise ValueError(f"labels {labels!r}: 'uniform' or 'learnable'")
    return x, y
