"""fp64 numpy reference of the strided test_cnn (mpiLAPI.py:178-195) for the topclass
population tests: forward, backward, loss, update.  TEST INFRASTRUCTURE ONLY.

    Conv2D(32, k, strides 3, valid, relu) x 2 -> MaxPool 2x2 (floor) -> Dropout(dropout / 2)
    -> Flatten (NHWC) -> Dense(128, relu) -> Dropout(dropout) -> Dense(classes, softmax)

The dropout hash, the softmax and the optimizer rules are oracle/cnn.py's; the losses are
its ``bce_loss_and_grad`` / ``cce_loss_and_grad`` with the class count in place of 10.  A
rate outside (0, 1) is the identity (Keras 2 ``Dropout.call``).  The rates are the float32
the C ABI carries (MpoTcSpec.dropout), halved for layer 0.
"""
import numpy as np

from oracle import cnn as OC

STRIDE, FILTERS, DENSE = 3, 32, 128
EPS = OC.BCE_EPS


def geometry(shape, k):
    H, W, C = shape
    out = lambda n: (n - k) // STRIDE + 1
    H1, W1 = out(H), out(W)
    H2, W2 = out(H1), out(W1)
    return dict(H=H, W=W, C=C, k=k, H1=H1, W1=W1, H2=H2, W2=W2, Hp=H2 // 2, Wp=W2 // 2,
                K1=(H2 // 2) * (W2 // 2) * FILTERS)


def im2col(x, k):
    """[B,H,W,C] -> ([B*Ho*Wo, k*k*C] in (ky, kx, c) order, (B, Ho, Wo)), stride 3, valid."""
    B, H, W, C = x.shape
    Ho, Wo = (H - k) // STRIDE + 1, (W - k) // STRIDE + 1
    sb, sh, sw, sc = x.strides
    v = np.lib.stride_tricks.as_strided(x, (B, Ho, Wo, k, k, C), (sb, STRIDE * sh, STRIDE * sw, sh, sw, sc),
                                        writeable=False)
    return v.reshape(B * Ho * Wo, k * k * C), (B, Ho, Wo)


def conv_fwd(x, w, b):
    k, _, C, F = w.shape
    cols, (B, Ho, Wo) = im2col(x, k)
    return (cols @ w.reshape(k * k * C, F) + b).reshape(B, Ho, Wo, F), cols


def conv_dgrad(dz, x_shape, w):
    """Input gradient: zeros where no window reaches, sums where several do."""
    k, _, C, F = w.shape
    B, Ho, Wo, _ = dz.shape
    dcols = (dz.reshape(-1, F) @ w.reshape(k * k * C, F).T).reshape(B, Ho, Wo, k, k, C)
    dx = np.zeros(x_shape, dtype=dz.dtype)
    for ky in range(k):
        for kx in range(k):
            dx[:, ky:ky + STRIDE * Ho:STRIDE, kx:kx + STRIDE * Wo:STRIDE, :] += dcols[:, :, :, ky, kx, :]
    return dx


def maxpool_fwd(a):
    B, H, W, F = a.shape
    Hp, Wp = H // 2, W // 2
    v = a[:, :2 * Hp, :2 * Wp, :].reshape(B, Hp, 2, Wp, 2, F).transpose(0, 1, 3, 5, 2, 4).reshape(B, Hp, Wp, F, 4)
    arg = np.argmax(v, axis=-1)          # first maximum in (dy, dx) row-major order
    return np.take_along_axis(v, arg[..., None], -1)[..., 0], arg


def maxpool_bwd(dpool, arg, shape):
    B, H, W, F = shape
    Hp, Wp = H // 2, W // 2
    onehot = (np.arange(4)[None, None, None, None, :] == arg[..., None]) * dpool[..., None]
    d = onehot.reshape(B, Hp, Wp, F, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, 2 * Hp, 2 * Wp, F)
    out = np.zeros(shape, dtype=dpool.dtype)
    out[:, :2 * Hp, :2 * Wp, :] = d
    return out


def bce_loss_and_grad(prob, onehot):
    B, nc = prob.shape
    pc = np.clip(prob, EPS, 1 - EPS)
    loss = (-(onehot * np.log(pc) + (1 - onehot) * np.log(1 - pc))).mean(axis=1)
    inside = (prob > EPS) & (prob < 1 - EPS)
    dp = np.where(inside, (pc - onehot) / (pc * (1 - pc)), 0.0) / (nc * B)
    return loss, prob * (dp - (dp * prob).sum(axis=1, keepdims=True))


LOSSES = {"binary_crossentropy": bce_loss_and_grad, "categorical_crossentropy": OC.cce_loss_and_grad}


def dropout_rates(dropout):
    """(layer 0, layer 1) rates as the device computes them from the float32 rate; None = identity."""
    r = np.float32(dropout)
    r0, r1 = float(r / np.float32(2)), float(r)
    return (r0 if 0 < r0 < 1 else None), (r1 if 0 < r1 < 1 else None)


def dropout_mult(seed, step, layer, n, rate):
    if rate is None:
        return np.ones(n)
    inv = float(np.float32(1) / (np.float32(1) - np.float32(rate)))
    return OC.dropout_keep(seed, step, layer, n, rate) * inv


class TopclassRef:
    """One member.  ``params``: dict of arrays in Keras shapes."""

    def __init__(self, shape, classes, k, params, lr=1e-3, dropout=0.5, seed=0, loss="categorical_crossentropy",
                 optimizer="adam"):
        self.g = geometry(shape, k)
        self.classes = classes
        self.params = {n: np.array(v, dtype=np.float64) for n, v in params.items()}
        self.lr, self.dropout, self.seed = float(np.float32(lr)), dropout, seed
        self.loss_fn, self.optimizer = LOSSES[loss], optimizer
        self.m = {n: np.zeros_like(v) for n, v in self.params.items()}
        self.v = {n: np.zeros_like(v) for n, v in self.params.items()}
        self.t = 0

    def forward(self, x, y, step=None, train=True, masks=None):
        """``masks`` = (m1 [B,K1], m2 [B,128]) overrides the hash masks (fixed multipliers)."""
        P = self.params
        B = x.shape[0]
        x = x.astype(np.float64)
        z1, c1 = conv_fwd(x, P["w1"], P["b1"])
        a1 = np.maximum(z1, 0)
        z2, c2 = conv_fwd(a1, P["w2"], P["b2"])
        a2 = np.maximum(z2, 0)
        pool, arg = maxpool_fwd(a2)
        flat = pool.reshape(B, -1)
        if masks is not None:
            m1, m2 = masks
        elif train:
            r0, r1 = dropout_rates(self.dropout)
            m1 = dropout_mult(self.seed, step, 0, flat.size, r0).reshape(flat.shape)
            m2 = dropout_mult(self.seed, step, 1, B * DENSE, r1).reshape(B, DENSE)
        else:
            m1, m2 = np.ones_like(flat), np.ones((B, DENSE))
        pd = flat * m1
        h = np.maximum(pd @ P["w3"] + P["b3"], 0)
        hd = h * m2
        prob = OC.softmax(hd @ P["w4"] + P["b4"])
        onehot = np.eye(self.classes)[np.asarray(y)]
        loss, dz3 = self.loss_fn(prob, onehot)
        cache = dict(x=x, c1=c1, a1=a1, c2=c2, a2=a2, arg=arg, pd=pd, m1=m1, h=h, m2=m2, hd=hd, dz3=dz3,
                     pool_shape=pool.shape)
        return float(loss.mean()), loss, prob, cache

    def backward(self, cache, abs_terms=False, decisions=None):
        """Gradients; with ``abs_terms`` also sum |terms| of every gradient's final
        contraction (|cols|^T |dz|).  ``decisions`` overrides the forward's discrete
        choices (``arg``, ``a1_pos`` / ``a2_pos`` / ``h_pos``) with another implementation's,
        as oracle/cnn.py's does."""
        P, c = self.params, dict(cache)
        decisions = decisions or {}
        arg = decisions.get("arg", c["arg"])
        gate = {n: decisions.get(n + "_pos", c[n] > 0) for n in ("a1", "a2", "h")}
        F = FILTERS
        g = {"w4": c["hd"].T @ c["dz3"], "b4": c["dz3"].sum(0)}
        dh = (c["dz3"] @ P["w4"].T) * c["m2"] * gate["h"]
        g["w3"], g["b3"] = c["pd"].T @ dh, dh.sum(0)
        dpool = ((dh @ P["w3"].T) * c["m1"]).reshape(c["pool_shape"])
        dz2 = maxpool_bwd(dpool, arg, c["a2"].shape) * gate["a2"]
        g["w2"], g["b2"] = (c["c2"].T @ dz2.reshape(-1, F)).reshape(P["w2"].shape), dz2.reshape(-1, F).sum(0)
        dz1 = conv_dgrad(dz2, c["a1"].shape, P["w2"]) * gate["a1"]
        g["w1"], g["b1"] = (c["c1"].T @ dz1.reshape(-1, F)).reshape(P["w1"].shape), dz1.reshape(-1, F).sum(0)
        self.last = dict(dz1=dz1, dz2=dz2)
        if not abs_terms:
            return g
        A = np.abs
        absg = {"w4": A(c["hd"]).T @ A(c["dz3"]), "b4": A(c["dz3"]).sum(0), "w3": A(c["pd"]).T @ A(dh),
                "b3": A(dh).sum(0),
                "w2": (A(c["c2"]).T @ A(dz2).reshape(-1, F)).reshape(P["w2"].shape), "b2": A(dz2).reshape(-1, F).sum(0),
                "w1": (A(c["c1"]).T @ A(dz1).reshape(-1, F)).reshape(P["w1"].shape), "b1": A(dz1).reshape(-1, F).sum(0)}
        return g, absg

    def update(self, grads, b1=0.9, b2=0.999, eps=1e-8):
        """Keras Adam / SGD (oracle/cnn.py TrialOracle.adam / sgd)."""
        self.t += 1
        if self.optimizer == "sgd":
            for n in self.params:
                self.params[n] = self.params[n] - self.lr * grads[n]
            return
        lr_t = self.lr * np.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)
        for n in self.params:
            self.m[n] = b1 * self.m[n] + (1 - b1) * grads[n]
            self.v[n] = b2 * self.v[n] + (1 - b2) * grads[n] * grads[n]
            self.params[n] = self.params[n] - lr_t * self.m[n] / (np.sqrt(self.v[n]) + eps)

    def train_step(self, x, y, step):
        loss, _, _, cache = self.forward(x, y, step=step, train=True)
        self.update(self.backward(cache))
        return loss

    def eval_batch(self, x, y):
        """(sum of per-sample losses, correct count) of one batch, no dropout."""
        _, l, prob, _ = self.forward(x, y, train=False)
        return float(l.sum()), int((np.argmax(prob, axis=1) == np.asarray(y)).sum())
