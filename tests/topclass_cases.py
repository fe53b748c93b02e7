"""Case table of the topclass population GPU tests (tests/test_topclass_gpu.py); its
coverage is asserted without a GPU by tests/test_topclass_abi.py.

A case is one population: an input shape, a class count, a batch and members
(kernel_size, dropout, loss, optimizer).  The smallest legal shape of a kernel size is
H = W = 4 k + 6: conv1 gives k + 3, conv2 gives 2 (the pool needs 2 x 2).
"""
from dataclasses import dataclass

BCE, CCE = "binary_crossentropy", "categorical_crossentropy"


@dataclass(frozen=True)
class Case:
    name: str
    shape: tuple
    classes: int
    batch: int
    members: tuple            # (kernel_size, dropout, loss, optimizer)
    n_samples: int = 0        # 0: the batch


def _smallest(k):
    C = 5 if k % 2 else 1                   # k = 1 with C = 5: K = 5, a padded MFMA k-step
    classes = 3 if k % 3 else 5
    batch = (1, 3, 7)[k % 3]
    dropout = (0.0, 0.3, 1.0)[(k // 2) % 3]
    return Case(f"k{k}_smallest", (4 * k + 6, 4 * k + 6, C), classes, batch,
                ((k, dropout, CCE if k % 2 else BCE, "adam"),))


CASES = [_smallest(k) for k in range(1, 10)] + [
    # residues (in - k) % 3 of (conv1 h, conv1 w, conv2 h, conv2 w) and conv2 outputs in the comments
    Case("k2_res_1_2_2_0", (21, 25, 5), 3, 3, ((2, 0.3, CCE, "adam"),)),          # conv2 2 x 3
    Case("k4_res_2_1_1_2", (27, 29, 1), 5, 7, ((4, 1.0, BCE, "adam"),)),          # conv2 2 x 2
    Case("k2_res_1_0_2_1", (21, 17, 5), 3, 1, ((2, 0.0, BCE, "sgd"),)),           # conv2 2 x 2
    Case("k3_res_0_2_1_2", (30, 26, 3), 3, 3, ((3, 0.3, CCE, "sgd"),)),           # conv2 3 x 2
    # members of different k in one population: conv2 5x4, 4x4, 4x3, 3x2
    Case("mixed_k_1_2_3_5", (40, 34, 5), 3, 3,
         ((1, 0.3, CCE, "adam"), (2, 1.0, BCE, "adam"), (3, 0.0, CCE, "sgd"), (5, 0.3, BCE, "adam"))),
    # the reference shape (option3's LCD-jet images)
    Case("reference_shape", (150, 94, 5), 3, 4, ((1, 0.3, CCE, "adam"), (3, 0.5, CCE, "adam"), (6, 1.0, BCE, "adam"))),
]

# the second step's gradients: k = 1 leaves a1 pixels in no conv2 window, k = 5 puts them in up to 4
SECOND_STEP = Case("second_step_k1_k5", (26, 28, 5), 3, 3, ((1, 0.3, CCE, "adam"), (5, 0.3, CCE, "adam")), n_samples=6)

# 6 train steps and one eval batch
TRAJECTORY = Case("trajectory", (30, 26, 5), 3, 5,
                  ((3, 0.3, BCE, "adam"), (2, 0.5, CCE, "adam"), (4, 0.3, CCE, "sgd")), n_samples=40)

# a member alone and inside a population of 5 with mixed k: (case, index of the member)
ISOLATION = [
    (Case("isolation_b3", (40, 34, 5), 3, 3,
          ((1, 0.3, CCE, "adam"), (5, 0.3, BCE, "adam"), (3, 0.5, CCE, "adam"), (2, 0.0, CCE, "sgd"), (3, 1.0, BCE, "adam")),
          n_samples=9), 2),
    (Case("isolation_b100", (22, 18, 2), 3, 100,
          ((2, 0.3, CCE, "adam"), (1, 0.3, BCE, "adam"), (3, 0.5, CCE, "adam"), (1, 0.0, CCE, "sgd"), (3, 1.0, BCE, "adam")),
          n_samples=300), 2),
]


def residues(case):
    """{(conv, axis): residue} per member, conv2 output sizes per member."""
    out = []
    for (k, *_rest) in case.members:
        H, W, _ = case.shape
        H1, W1 = (H - k) // 3 + 1, (W - k) // 3 + 1
        out.append(dict(k=k, c1h=(H - k) % 3, c1w=(W - k) % 3, c2h=(H1 - k) % 3, c2w=(W1 - k) % 3,
                        H2=(H1 - k) // 3 + 1, W2=(W1 - k) // 3 + 1))
    return out
