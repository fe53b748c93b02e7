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

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .population import train_folds

FILTERS = 32
DENSE = 128
STRIDE = 3
PARAM_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
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

    def options(self):
        """MpoTcSpec.options bits; raises for a loss / optimizer the kernels do not implement."""
        try:
            return _lib.LOSS_CODES[self.loss] | _lib.OPT_CODES[self.optimizer]
        except KeyError:
            raise ValueError(f"unsupported loss / optimizer {self.loss!r} / {self.optimizer!r}: the population "
                             f"kernels implement losses {sorted(_lib.LOSS_CODES)} and optimizers "
                             f"{sorted(_lib.OPT_CODES)}") from None

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


def glorot_uniform_init(spec: TopclassSpec, seed: int):
    """Keras defaults: glorot_uniform kernels, zero biases (float32)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in spec.param_shapes().items():
        if name.startswith("w"):
            rf = shape[0] * shape[1] if len(shape) == 4 else 1
            fan_in, fan_out = rf * shape[-2], rf * shape[-1]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            out[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        else:
            out[name] = np.zeros(shape, dtype=np.float32)
    return out


class TopclassPopulation:
    """A population of test_cnn members on one input shape, resident on one GPU.
    The ``PopulationEngine`` surface without ``set_active``: a stopping rule still ends
    members' histories, the stopped members keep stepping (``train_folds``)."""

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
        self.n = len(self.specs)
        self.batch = int(batch)
        self.device = torch.device(device if device is not None else "cuda")
        L = lib()
        arr = (_lib.MpoTcSpec * self.n)()
        for i, s in enumerate(self.specs):
            arr[i] = _lib.MpoTcSpec(int(s.kernel_size), float(s.lr), float(s.dropout), int(s.seed) & 0xFFFFFFFF,
                                    s.options())
        h = ctypes.c_void_p()
        H, W, C = self.input_shape
        check(L.mpo_tc_create(arr, self.n, self.batch, H, W, C, self.classes, ctypes.byref(h)), "mpo_tc_create")
        self._h = h
        sz = _lib.MpoPopSizes()
        check(L.mpo_tc_sizes(h, ctypes.byref(sz)), "mpo_tc_sizes")
        self.n_params = int(sz.n_params)
        self.layout = []
        offs = (ctypes.c_int64 * 9)()
        for i in range(self.n):
            check(L.mpo_tc_param_layout(h, i, offs), "mpo_tc_param_layout")
            self.layout.append([int(v) for v in offs])
        self.act_layout = []
        aoffs = (ctypes.c_int64 * 12)()
        for i in range(self.n):
            check(L.mpo_tc_act_layout(h, i, aoffs), "mpo_tc_act_layout")
            self.act_layout.append(dict(zip(ACT_NAMES, [int(v) for v in aoffs])))
        dev = self.device
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.grads = torch.zeros_like(self.params)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.act = torch.zeros(int(sz.act_floats), dtype=torch.float32, device=dev)
        self.tables = torch.empty(int(sz.table_bytes), dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.val_loss_sum = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.val_correct = torch.zeros(self.n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(L.mpo_tc_bind(h, ptr(self.params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v),
                                ptr(self.act), ptr(self.tables), _lib.stream_handle(dev)), "mpo_tc_bind")
        if init is None:
            init = [glorot_uniform_init(s, init_seed + i) for i, s in enumerate(self.specs)]
        for i, p in enumerate(init):
            self.set_params(i, p)
        self.step_count = 0

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().mpo_tc_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- parameters -------------------------------------------------------------
    def _slices(self, i):
        o = self.layout[i]
        shapes = self.specs[i].param_shapes()
        return {n: (o[j], shapes[n]) for j, n in enumerate(PARAM_NAMES)}

    def set_params(self, i, params):
        for n, (off, shape) in self._slices(i).items():
            a = np.ascontiguousarray(np.asarray(params[n], dtype=np.float32).reshape(shape))
            self.params[off:off + a.size].copy_(torch.from_numpy(a.reshape(-1)))

    def _read(self, arena, i):
        host = arena[self.layout[i][0]:self.layout[i][8]].cpu().numpy()
        base = self.layout[i][0]
        return {n: host[off - base:off - base + int(np.prod(shape))].reshape(shape).copy()
                for n, (off, shape) in self._slices(i).items()}

    def get_params(self, i):
        return self._read(self.params, i)

    def get_grads(self, i):
        """Member i's gradients of the last train step (Keras shapes)."""
        return self._read(self.grads, i)

    def activation(self, i, name, shape, dtype=torch.float32):
        """Copy of member i's activation tensor ``name`` of the last step (diagnostics /
        tests); the pool argmax ``am`` is int32 (2 dy + dx)."""
        off = self.act_layout[i][name]
        return self.act[off:off + int(np.prod(shape))].view(dtype).reshape(shape).cpu().numpy()

    def reset_optimizer(self):
        self.adam_m.zero_()
        self.adam_v.zero_()
        self.step_count = 0

    # -- steps --------------------------------------------------------------------
    def _check(self, x, labels, order, row0):
        if tuple(x.shape[1:]) != self.input_shape or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"x must be contiguous float32 [n, {self.input_shape}], got {tuple(x.shape)} {x.dtype}")
        if labels.dtype != torch.int32 or labels.shape[0] != x.shape[0] or order.dtype != torch.int32:
            raise ValueError("labels [n] and order [n_members, L] must be int32")
        if order.dim() != 2 or order.shape[0] != self.n or not order.is_contiguous() or row0 < 0 \
                or row0 + self.batch > order.shape[1]:
            raise ValueError(f"order {tuple(order.shape)} does not hold rows [{row0}, {row0 + self.batch}) of "
                             f"{self.n} members")

    def train_step(self, x, labels, order, row0, step=None):
        """x [n,H,W,C] f32, labels [n] i32, order [n_members, L] i32 (device)."""
        self._check(x, labels, order, int(row0))
        step = self.step_count if step is None else int(step)
        with torch.cuda.device(self.device):
            check(lib().mpo_tc_train_step(self._h, ptr(x), ptr(labels), ptr(order), int(order.shape[1]), int(row0),
                                          step, ptr(self.loss), _lib.stream_handle(self.device)),
                  "mpo_tc_train_step")
        self.step_count = step + 1
        return self.loss

    def eval_reset(self):
        self.val_loss_sum.zero_()
        self.val_correct.zero_()

    def eval_step(self, x, labels, order, row0):
        self._check(x, labels, order, int(row0))
        with torch.cuda.device(self.device):
            check(lib().mpo_tc_eval_step(self._h, ptr(x), ptr(labels), ptr(order), int(order.shape[1]), int(row0),
                                         ptr(self.val_loss_sum), ptr(self.val_correct),
                                         _lib.stream_handle(self.device)), "mpo_tc_eval_step")

    def fit_folds(self, x, labels, folds, n_fold, epochs, record_train_loss=False, holdout=None, progress=None,
                  stopping=None, retire_stopped=False):
        """As :meth:`PopulationEngine.fit_folds` (population.train_folds); there is no
        ``set_active`` here, so ``retire_stopped`` changes nothing."""
        return train_folds(self, x, labels, folds, n_fold, epochs, record_train_loss, holdout, progress, stopping,
                           retire_stopped=retire_stopped)


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
